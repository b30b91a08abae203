# Prints what tick_ab.sh left under bench_out/.
tail -n 3 bench_out/par.log
grep -hv amdgpu.ids bench_out/stamps_C2.txt bench_out/stamps_C3.txt
for f in C2 C3 C4n C4; do
  [ -f bench_out/$f.json ] || continue
  python - "$f" <<'PY'
import json, sys
f = sys.argv[1]
d = json.loads(open(f"bench_out/{f}.json").read().strip().splitlines()[-1])
print(f, round(d["value"] / 1e6, 1), "M", d["ms_per_step"], d["kernel_ms"], d["roofline"]["avg_launch_ms"])
PY
done
