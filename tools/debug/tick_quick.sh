# tick change check: parity tests (rollouts, full size, item stress, wrapper), phase stamps for
# C2 / C3 / C4, then C2 / C3 / C4-native / C5 bench lines
cd "$(dirname "$0")/../.." && export TMPDIR=/tmp && mkdir -p bench_out/tq && set -o pipefail
timeout -k 10 400 python -u -m pytest -x -q --timeout 200 --timeout-method thread tests/test_gpu_parity.py \
  tests/test_gpu_fullsize.py tests/test_gpu_wrapper.py > bench_out/tq/tests.log 2>&1 || { echo TESTS FAILED; tail -30 bench_out/tq/tests.log; exit 1; }
tail -1 bench_out/tq/tests.log
STAMPS_STAGGER=64 timeout -k 10 150 python tools/stamps.py C4 512 40 > bench_out/tq/stamps_C4.txt 2>&1 || exit 1
STAMPS_STAGGER=64 timeout -k 10 150 python tools/stamps.py C3 1024 40 > bench_out/tq/stamps_C3.txt 2>&1 || exit 1
STAMPS_STAGGER=64 timeout -k 10 150 python tools/stamps.py C2 128 40 > bench_out/tq/stamps_C2.txt 2>&1 || exit 1
for c in "C2" "C3" "C4 --obs native" "C5"; do
  n=$(echo $c | tr -d ' -')
  timeout -k 10 150 python bench.py --full --config $c --no-cpu-baseline --no-extras > bench_out/tq/$n.json 2> bench_out/tq/$n.err || { echo BENCH $c failed; tail -3 bench_out/tq/$n.err; exit 1; }
done
echo OK
