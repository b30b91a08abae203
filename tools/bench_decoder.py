"""The fused decoder (`decoder.decoder_heads`, SPEC.md §23) against the composed path it replaces, on one
GPU: `item_logits` x 2, `player_logits`, `cat` with the four dense heads' logits and `masked_heads`, the
twelve nmmo heads over flat float32 obs rows (stride 23,987 floats) read in place. Both paths get the
same dense logits and the same projected queries pq [N, 8, 40]; what differs is the decoder alone.

Masks are DESIGN.md §3.15's, generated as tools/bench_heads.py --pointer generates them: "sparse" (what
the workload produces: the no-op plus on average 10 entities, 4 inventory slots and 6 market listings,
at most 8, per head; dense heads 30 % legal) and "all" (every entry legal).

Per row count (default 4,096) and mask it reports, as the median and min..max over `repeats` windows
of `iters` back-to-back calls (device events; the two variants alternate window by window in one
process after warm-up), and with `torch.cuda.max_memory_allocated` over one call on top of what was
allocated before it:
  forward_sample     sampling under no_grad
  forward_given      the given actions under no_grad
  forward_backward   the given actions, forward and backward to the dense logits and to pq
Where the two ranges overlap the line says "no difference shown".

Usage (GPU box): python tools/bench_decoder.py [rows ...] [--iters N] [--repeats N] [--out FILE]
"""

import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from nmmo_amd import layout  # noqa: E402
from nmmo_amd.decoder import decoder_heads  # noqa: E402
from nmmo_amd.heads import masked_heads  # noqa: E402
from nmmo_amd.item import item_logits  # noqa: E402
from nmmo_amd.player import player_logits  # noqa: E402

OBS_ELEMS = 23987
SETS = (("Entity", "entity", layout.PLAYER_N_OBS, 31), ("Inventory", "item", layout.INVENTORY_N_OBS, 16),
        ("Market", "item", layout.MARKET_N_OBS, 16))
HEAD_SET = [-1, 0, 2, 1, 1, 0, -1, 0, -1, 1, -1, 1]
DIMS = list(layout.ACTION_DIMS)


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


def make_obs(rows, density, g):
    lay = layout.flat_layout()
    obs = torch.zeros((rows, OBS_ELEMS), dtype=torch.float32, device="cuda")
    for name, _, R, cols in SETS:
        x = torch.randint(0, 160, (rows, R, cols), device="cuda", generator=g).float()
        x[:, :, 1] = torch.randint(0, 5, (rows, R), device="cuda", generator=g).float()
        if cols == 16:
            x[:, :, 14] = torch.randint(0, 2, (rows, R), device="cuda", generator=g).float()
        obs[:, lay[name].offset:lay[name].offset + R * cols] = x.reshape(rows, -1)
    off = [0]
    for n in DIMS:
        off.append(off[-1] + n)
    rand = lambda *shape: torch.rand(shape, device="cuda", generator=g)  # noqa: E731
    for k, n in enumerate(DIMS):
        if density == "all":
            obs[:, off[k]:off[k + 1]] = 1.0
        elif HEAD_SET[k] < 0:
            obs[:, off[k]:off[k + 1]] = (rand(rows, n) < 0.3).float()
        else:
            want = {0: 10.0, 1: 4.0, 2: 6.0}[HEAD_SET[k]]  # expected legal candidates (market: <= 8)
            legal = rand(rows, n - 1) < want / (n - 1)
            if HEAD_SET[k] == 2:
                legal &= torch.cumsum(legal, 1) <= 8
            obs[:, off[k]:off[k + 1] - 1] = legal.float()
            obs[:, off[k + 1] - 1] = 1.0  # the no-op
    return obs, off


def bench_rows(rows, density, iters, repeats):
    g = torch.Generator(device="cuda").manual_seed(1)
    obs, off = make_obs(rows, density, g)
    lay = layout.flat_layout()
    views = [obs[:, lay[name].offset:lay[name].offset + R * cols] for name, _, R, cols in SETS]
    pointer = [k for k, s in enumerate(HEAD_SET) if s >= 0]
    n_dense = sum(n for n, s in zip(DIMS, HEAD_SET) if s < 0)
    dense0 = torch.randn((rows, n_dense), device="cuda", generator=g)
    pq0 = torch.randn((rows, len(pointer), 40), device="cuda", generator=g) / 256.0
    w_lp = torch.randn(rows, device="cuda", generator=g)

    def fused(dense, pq, action):
        sets = [(v, rule) for v, (_, rule, _, _) in zip(views, SETS)]
        return decoder_heads(dense, pq, sets, HEAD_SET, obs, DIMS, action, seed=1)

    def composed(dense, pq, action):
        parts, d = [None] * len(DIMS), 0
        for k, s in enumerate(HEAD_SET):
            if s < 0:
                parts[k] = dense[:, d:d + DIMS[k]]
                d += DIMS[k]
        for s, (_, rule, R, _) in enumerate(SETS):
            ks = [k for k in pointer if HEAD_SET[k] == s]
            slots = pq[:, [pointer.index(k) for k in ks], :40 if rule == "entity" else 36]
            fn = player_logits if rule == "entity" else item_logits
            lg = fn(views[s], slots, obs, [off[k] for k in ks], set_rows=R)
            for i, k in enumerate(ks):
                parts[k] = lg[:, i * (R + 1):(i + 1) * (R + 1)]
        return masked_heads(torch.cat(parts, 1), obs, DIMS, action, seed=1)

    paths = {"fused": fused, "composed": composed}
    with torch.no_grad():
        actions = fused(dense0, pq0, None)[0]
        same_actions = bool(torch.equal(actions, composed(dense0, pq0, None)[0]))
        lp = [p(dense0, pq0, actions)[1] for p in paths.values()]
    legal = sum(float((obs[:, off[k]:off[k + 1] - 1] > 0).sum()) for k in pointer) / rows

    def call(name, part):
        path = paths[name]

        def fn():
            if part == "forward_sample":
                with torch.no_grad():
                    return path(dense0, pq0, None)
            if part == "forward_given":
                with torch.no_grad():
                    return path(dense0, pq0, actions)
            dense, pq = dense0.clone().requires_grad_(True), pq0.clone().requires_grad_(True)
            _, logp, ent = path(dense, pq, actions)
            ((logp * w_lp).sum() + 0.01 * ent.sum()).backward()
            return dense.grad, pq.grad
        return fn

    out = {"rows": rows, "mask": density, "iters": iters, "repeats": repeats,
           "legal_candidates_per_row": round(legal, 2), "sampled_actions_equal": same_actions,
           "logprob_bits_equal": bool(torch.equal(lp[0].view(torch.int32), lp[1].view(torch.int32)))}
    for part in ("forward_sample", "forward_given", "forward_backward"):
        fns = {name: call(name, part) for name in paths}
        for fn in fns.values():  # warm up: code objects, the allocator
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in paths}
        for _ in range(repeats):
            for name in paths:
                times[name].append(window(fns[name], iters))
        r = {}
        for name in paths:
            r[name + "_us"] = {"median": round(statistics.median(times[name]), 1), "min": round(min(times[name]), 1),
                               "max": round(max(times[name]), 1)}
            r[name + "_peak_bytes"] = peak(fns[name])
        f, c = r["fused_us"], r["composed_us"]
        if f["max"] < c["min"] or c["max"] < f["min"]:
            r["verdict"] = f"composed / fused = {c['median'] / f['median']:.2f} (ranges apart)"
        else:
            r["verdict"] = "no difference shown"
        out[part] = r
    return out


def main():
    args = sys.argv[1:]
    opt = {"--iters": 10, "--repeats": 7, "--out": None}
    rows = []
    while args:
        a = args.pop(0)
        if a in opt:
            v = args.pop(0)
            opt[a] = v if a == "--out" else int(v)
        else:
            rows.append(int(a))
    if not torch.cuda.is_available():
        raise SystemExit("bench_decoder.py measures on a GPU: none found")
    res = [bench_rows(n, density, opt["--iters"], opt["--repeats"]) for n in rows or [4096] for density in ("sparse", "all")]
    text = "\n".join(json.dumps(r) for r in res)
    print(text)
    if opt["--out"]:
        os.makedirs(os.path.dirname(os.path.abspath(opt["--out"])), exist_ok=True)
        with open(opt["--out"], "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
