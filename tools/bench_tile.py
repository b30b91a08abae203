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
from nmmo_amd.tile import ROW, TileEncoder, n_chunks_for  # noqa: E402

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
    enc = {True: TileEncoder(256, fused=True).cuda(), False: TileEncoder(256, fused=False).cuda()}
    enc[False].load_state_dict(enc[True].state_dict())
    w_out = torch.randn((rows, 256), device="cuda", generator=g)
    w_c1 = torch.randn((rows, 32, 13, 13), device="cuda", generator=g)

    def call(fused, part, grad):
        m = enc[fused]

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
           "embedding_bytes_per_row_unfused": 96 * 225 * 4, "index_bytes_per_row_fused": ROW}
    with torch.no_grad():
        a, b = enc[True].conv1(obs, off), enc[False].conv1(obs, off)
        out["conv1_max_abs_difference"] = float((a - b).abs().max())
    for part in ("conv1", "encoder"):
        for grad in (False, True):
            fns = {fused: call(fused, part, grad) for fused in (True, False)}
            for fn in fns.values():  # warm up: code objects, MIOpen's algorithm search, the allocator
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {True: [], False: []}
            for _ in range(repeats):
                for fused in (True, False):
                    times[fused].append(window(fns[fused], iters))
            key = f"{part}_{'forward_backward' if grad else 'forward_no_grad'}"
            r = {}
            for fused, name in ((True, "fused"), (False, "unfused")):
                r[name + "_us"] = {"median": round(statistics.median(times[fused]), 1),
                                   "min": round(min(times[fused]), 1), "max": round(max(times[fused]), 1)}
                r[name + "_peak_bytes"] = peak(fns[fused])
            r["unfused_over_fused_time"] = round(r["unfused_us"]["median"] / r["fused_us"]["median"], 2)
            r["unfused_over_fused_peak"] = round(r["unfused_peak_bytes"] / max(1, r["fused_peak_bytes"]), 2)
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
