"""The fused tile encoder (nmmo_amd/tile.py, SPEC.md §19) against the unfused torch chain it
replaces, on one GPU: the same `TileEncoder` module with `fused=True` and `fused=False`, the same
weights, the Tile section read from flat obs rows (stride 23,987 floats) whose coordinates and
materials are what a rollout produces (a 15 x 15 window at a random map position, materials 0..15).

Per row count (default 1,024, one minibatch, and 16,384) it reports, for forward under `no_grad`
and for forward + backward: the median and the min..max over `repeats` windows of `iters`
back-to-back calls (device events; the two variants alternate window by window), and
`torch.cuda.max_memory_allocated` over one call on top of what was allocated before it. "conv1"
rows time only the part the kernel replaces (embedding + tile_conv_1 + ReLU), "encoder" rows the
whole module. Bytes per row are the algorithmic ones: the unfused chain writes and keeps the
[96, 15, 15] float32 embedding tensor (86,400 B), the fused one the 675 index bytes.

The "encoder" rows carry a third variant, `fused=True, fused_conv2=True` (SPEC.md §22: the second
convolution in the same kernel, the [32, 13, 13] activation of 21,632 B per row never written), in
the same windows and alternation, as `fused_conv2_*` keys; `encoder_max_abs_difference` holds the
three paths' pairwise largest output differences.

Usage (GPU box): python tools/bench_tile.py [rows ...] [--iters N] [--repeats N] [--out FILE]
"""

import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from nmmo_amd import layout  # noqa: E402
from nmmo_amd.tile import ROW, TileEncoder, n_chunks_for, n_w2_parts_for  # noqa: E402

OBS_ELEMS = 23987


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters  # us per call


def peak(fn):
    """bytes `fn` allocates at its peak on top of what is allocated now"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def make_obs(rows, g):
    obs = torch.zeros((rows, OBS_ELEMS), dtype=torch.float32, device="cuda")
    off = layout.flat_layout()["Tile"].offset
    yy, xx = torch.meshgrid(torch.arange(15, device="cuda"), torch.arange(15, device="cuda"), indexing="ij")
    r0 = torch.randint(0, 160, (rows, 1), device="cuda", generator=g)
    c0 = torch.randint(0, 160, (rows, 1), device="cuda", generator=g)
    sec = torch.empty((rows, 225, 3), device="cuda")
    sec[:, :, 0] = r0 + yy.reshape(1, 225)
    sec[:, :, 1] = c0 + xx.reshape(1, 225)
    sec[:, :, 2] = torch.randint(0, 16, (rows, 225), device="cuda", generator=g).float()
    obs[:, off:off + ROW] = sec.reshape(rows, ROW)
    return obs, off


def bench_rows(rows, iters, repeats):
    g = torch.Generator(device="cuda").manual_seed(1)
    obs, off = make_obs(rows, g)
    torch.manual_seed(2)
    enc = {True: TileEncoder(256, fused=True).cuda(), False: TileEncoder(256, fused=False).cuda(),
           "conv2": TileEncoder(256, fused=True, fused_conv2=True).cuda()}
    enc[False].load_state_dict(enc[True].state_dict())
    enc["conv2"].load_state_dict(enc[True].state_dict())
    w_out = torch.randn((rows, 256), device="cuda", generator=g)
    w_c1 = torch.randn((rows, 32, 13, 13), device="cuda", generator=g)

    def call(variant, part, grad):
        m = enc[variant]

        def fn():
            if not grad:
                with torch.no_grad():
                    return m.conv1(obs, off) if part == "conv1" else m(obs, off)
            for p in m.parameters():
                p.grad = None
            y, w = (m.conv1(obs, off), w_c1) if part == "conv1" else (m(obs, off), w_out)
            (y * w).sum().backward()
        return fn

    out = {"rows": rows, "iters": iters, "repeats": repeats, "backward_chunks": n_chunks_for(rows),
           "backward_w2_parts": n_w2_parts_for(rows),
           "embedding_bytes_per_row_unfused": 96 * 225 * 4, "index_bytes_per_row_fused": ROW,
           "conv1_bytes_per_row_not_written_by_fused_conv2": 32 * 13 * 13 * 4}
    with torch.no_grad():
        a, b = enc[True].conv1(obs, off), enc[False].conv1(obs, off)
        out["conv1_max_abs_difference"] = float((a - b).abs().max())
        del a, b
        h = {name: enc[v](obs, off) for v, name in ((True, "fused"), (False, "unfused"), ("conv2", "fused_conv2"))}
        out["encoder_max_abs_difference"] = {f"{p}_vs_{q}": float((h[p] - h[q]).abs().max()) for p, q in
                                             (("fused_conv2", "fused"), ("fused_conv2", "unfused"), ("fused", "unfused"))}
        del h
    for part in ("conv1", "encoder"):
        # conv1() of the third variant is the second's: it enters the encoder rows only
        variants = [(True, "fused"), (False, "unfused")] + ([("conv2", "fused_conv2")] if part == "encoder" else [])
        for grad in (False, True):
            fns = {v: call(v, part, grad) for v, _ in variants}
            for fn in fns.values():  # warm up: code objects, MIOpen's algorithm search, the allocator
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {v: [] for v, _ in variants}
            for _ in range(repeats):
                for v, _ in variants:
                    times[v].append(window(fns[v], iters))
            key = f"{part}_{'forward_backward' if grad else 'forward_no_grad'}"
            r = {}
            for v, name in variants:
                r[name + "_us"] = {"median": round(statistics.median(times[v]), 1),
                                   "min": round(min(times[v]), 1), "max": round(max(times[v]), 1)}
                r[name + "_peak_bytes"] = peak(fns[v])
            r["unfused_over_fused_time"] = round(r["unfused_us"]["median"] / r["fused_us"]["median"], 2)
            r["unfused_over_fused_peak"] = round(r["unfused_peak_bytes"] / max(1, r["fused_peak_bytes"]), 2)
            if part == "encoder":
                r["fused_over_fused_conv2_time"] = round(r["fused_us"]["median"] / r["fused_conv2_us"]["median"], 2)
                r["fused_minus_fused_conv2_peak_bytes"] = r["fused_peak_bytes"] - r["fused_conv2_peak_bytes"]
                lo, hi = r["fused_conv2_us"], r["fused_us"]
                r["fused_conv2_vs_fused"] = ("faster" if lo["max"] < hi["min"] else
                                             "slower" if lo["min"] > hi["max"] else "tie")  # ranges must not overlap
            out[key] = r
    return out


def main():
    args = sys.argv[1:]
    opt = {"--iters": 20, "--repeats": 7, "--out": None}
    rows = []
    while args:
        a = args.pop(0)
        if a in opt:
            v = args.pop(0)
            opt[a] = v if a == "--out" else int(v)
        else:
            rows.append(int(a))
    if not torch.cuda.is_available():
        raise SystemExit("bench_tile.py measures on a GPU: none found")
    res = [bench_rows(n, opt["--iters"], opt["--repeats"]) for n in rows or [1024, 16384]]
    text = "\n".join(json.dumps(r) for r in res)
    print(text)
    if opt["--out"]:
        os.makedirs(os.path.dirname(os.path.abspath(opt["--out"])), exist_ok=True)
        with open(opt["--out"], "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
