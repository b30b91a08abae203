# wrapper-layer cost on each BASELINE config (same box A/B)
set -o pipefail
mkdir -p bench_out
for c in ${CONFIGS:-C2 C3 C4}; do
  for w in ${WRAPPERS:-none base neurips23_start_kit yaofeng}; do
    timeout -k 10 200 python bench.py --full --config $c --steps 100 --warmup 20 --no-cpu-baseline --wrapper $w > bench_out/bw_${c}_${w}.json 2>> bench_out/bw.err || exit 1
  done
done
