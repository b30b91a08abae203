"""Per-density kernel times of `tools/bench_heads.py ROWS ITERS --pointer` from the kernel trace of a
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_heads.py ROWS ITERS
--pointer` run (DESIGN.md §3.15's table; profiles/pointer_heads/kernel_times_4096.json).

The tool's launches come in a fixed order per mask density ("sparse", then "all"): one sampling
forward for the actions, 3 + ITERS sampling forwards, 3 + ITERS given-action forwards, 3 + ITERS
(given-action forward, backward) pairs, then the unfused torch chain, 3 + max(3, ITERS // 5)
sampling calls and as many forward + backward calls. The nmh_pointer_* kernels are told apart by
their position, the timed ones averaged; every other kernel between a density's last fused launch
and the next density's first is the torch chain's.

Usage: python tools/pointer_trace_summary.py <..._kernel_trace.csv> ITERS
"""

import csv
import json
import sys

WARM = 3  # bench_heads.timed()'s untimed calls


def main():
    path, iters = sys.argv[1], int(sys.argv[2])
    with open(path) as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    ev = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in rows]
    fused = [i for i, (name, _) in enumerate(ev) if "nmh_pointer" in name]
    per = 1 + 4 * (WARM + iters)  # fused launches per density
    assert len(fused) == 2 * per, (len(fused), per)
    torch_calls = WARM + max(3, iters // 5)
    mean = lambda v: round(sum(v) / len(v), 2)  # noqa: E731
    out = {}
    for d, density in enumerate(("sparse", "all")):
        mine = fused[d * per:(d + 1) * per]
        fwd = [ev[i][1] for i in mine if "forward" in ev[i][0]]
        bwd = [ev[i][1] for i in mine if "backward" in ev[i][0]]
        end = fused[(d + 1) * per] if d == 0 else len(ev)
        chain = [t for name, t in ev[mine[-1] + 1:end] if "nmh_" not in name]
        out[density] = {
            "forward_sample_us": mean(fwd[1 + WARM:1 + WARM + iters]),
            "forward_given_us": mean(fwd[1 + 2 * WARM + iters:1 + 2 * (WARM + iters)]),
            "forward_given_in_fb_us": mean(fwd[1 + 2 * (WARM + iters) + WARM:]),
            "backward_us": mean(bwd[WARM:]),
            "min_max_backward_us": [min(bwd), max(bwd)],
            "torch_chain_kernels": len(chain),
            "torch_chain_calls_each_of_sample_and_forward_backward": torch_calls,
            "torch_chain_kernel_us_per_sample_plus_forward_backward": round(sum(chain) / torch_calls, 1),
        }
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
