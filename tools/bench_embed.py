"""The fused embedded-set path (nmmo_amd/embed.py, SPEC.md §25) against the unfused torch chain it
replaces, on one GPU: the same `ReducedItemEncoder` and `ReducedPlayerEncoder` weights with `fused=True`
and `fused=False`, the Market and Entity sections read from flat obs rows (stride 23,987 floats).

Content "rollout": 0-8 listings and 1-20 entities per row, each legal for a head with probability
1/2. Content "all_legal": every one of the 1,024 listings and 100 entities is there and legal.

Per row count (default 1,024) and content it reports, as the median and min..max over `repeats`
windows of `iters` back-to-back calls (device events; the two variants alternate window by window),
and with `torch.cuda.max_memory_allocated` over one call on top of what was allocated before it:
  market   the pooled Market embedding [N, H] and the Buy head's logits [N, 1025]
  entity   the own row's my_agent [N, H] and the three entity heads' logits [N, 3 x 101]
each forward under no_grad and forward + backward to the layers, the tables and the queries (the
fused path's small torch matmuls, `pointer_query` among them, included), and the bytes each variant
must at least move per call: the sections read once plus, unfused, the [N, R, H] embedding written
and read once, so that a time can be set against the 6.29 TB/s float4 copy DESIGN §3.12 quotes.

Usage (GPU box): python tools/bench_embed.py [rows ...] [--iters N] [--repeats N] [--hidden H] [--out FILE]
"""

import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from nmmo_amd import layout  # noqa: E402
from nmmo_amd.embed import ENTITY, ITEM, ReducedItemEncoder, ReducedPlayerEncoder, embed_logits  # noqa: E402

OBS_ELEMS = 23987
COPY_BYTES_PER_S = 6.29e12  # the float4 copy kernel on this GPU
SETS = {"market": ("Market", ITEM, ("Buy.MarketItem",), 8),
        "entity": ("Entity", ENTITY, ("Attack.Target", "Give.Target", "GiveGold.Target"), 20)}


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


def make_obs(rows, content, g):
    """Flat obs rows whose Market and Entity sections, AgentId and the four heads' masks hold `content`."""
    lay = layout.flat_layout()
    obs = torch.zeros((rows, OBS_ELEMS), dtype=torch.float32, device="cuda")
    out = {}
    for key, (name, kind, heads_, most) in SETS.items():
        R, off = lay[name].shape[0], lay[name].offset
        x = torch.randint(0, 100, (rows, R, kind.cols), device="cuda", generator=g).float()
        x[:, :, 0] = (torch.arange(R, device="cuda") + 1).float()  # distinct ids
        if content == "rollout":  # the first k slots are filled, as the obs kernels write them
            k = torch.randint(1, most + 1, (rows, 1), device="cuda", generator=g)
            here = torch.arange(R, device="cuda").reshape(1, R) < k
            x = x * here.unsqueeze(-1)
        else:
            here = torch.ones((rows, R), dtype=torch.bool, device="cuda")
        obs[:, off:off + kind.cols * R] = x.reshape(rows, -1)
        offs = [lay[f"ActionTargets.{h}"].offset for h in heads_]
        for o in offs:
            legal = here if content == "all_legal" else here & (torch.rand((rows, R), device="cuda", generator=g) < 0.5)
            obs[:, o:o + R] = legal.float()
            obs[:, o + R] = 1.0  # the no-op
        out[key] = (obs[:, off:off + kind.cols * R], R, offs)
    obs[:, lay["AgentId"].offset] = 1.0
    return obs, out, lay["AgentId"].offset


def bench_set(key, rows, content, hidden, iters, repeats, g):
    obs, sets, o_id = make_obs(rows, content, g)
    sec, R, offs = sets[key]
    kind = SETS[key][1]
    cls = ReducedItemEncoder if key == "market" else ReducedPlayerEncoder
    torch.manual_seed(2)
    enc = {True: cls(hidden, hidden, fused=True).cuda(), False: cls(hidden, hidden, fused=False).cuda()}
    enc[False].load_state_dict(enc[True].state_dict())
    H = len(offs)
    q0 = torch.randn((rows, H, hidden), device="cuda", generator=g) / hidden ** 0.5
    w_a = torch.randn((rows, hidden), device="cuda", generator=g)
    w_lg = torch.cat([obs[:, o:o + R + 1] for o in offs], 1).clone()
    w_lg[:, R::R + 1] = 0
    w_lg = w_lg * torch.randn(w_lg.shape, device="cuda", generator=g)

    def encoded(fused):
        m = enc[fused]
        return m.pooled(sec, R) if key == "market" else m.my_agent(sec, obs[:, o_id], R)

    def logits(fused, q):
        m = enc[fused]
        if fused:
            return embed_logits(kind, sec, m.pointer_query(q), obs, offs, set_rows=R)
        emb = m.embed(sec, R)
        padded = torch.cat([emb, emb.new_zeros(rows, 1, hidden)], 1)
        return torch.cat([torch.matmul(padded, q[:, i].unsqueeze(-1)).squeeze(-1) for i in range(H)], 1)

    def call(fused, part):
        def fn():
            if part == "forward":
                with torch.no_grad():
                    return encoded(fused), logits(fused, q0)
            for p in enc[fused].parameters():
                p.grad = None
            q = q0.clone().requires_grad_(True)
            ((encoded(fused) * w_a).sum() + (logits(fused, q) * w_lg).sum()).backward()
            return q.grad
        return fn

    section = rows * R * kind.cols * 4
    out = {"set": key, "rows": rows, "content": content, "hidden": hidden, "iters": iters, "repeats": repeats,
           "legal_candidates_per_row": round(float((w_lg != 0).sum()) / rows, 2),
           "least_bytes_fused": section + rows * H * kind.query * 4,  # the section and the score tables, once each
           "least_bytes_unfused": section + 2 * rows * R * hidden * 4}  # ... and the embedding, written and read
    with torch.no_grad():
        legal = w_lg != 0
        out["legal_logits_max_abs_difference"] = float(((logits(True, q0) - logits(False, q0)) * legal).abs().max())
        out["encoded_max_abs_difference"] = float((encoded(True) - encoded(False)).abs().max())
    ga, gb = call(True, "forward_backward")(), call(False, "forward_backward")()
    out["query_gradient_max_abs_difference"] = float((ga - gb).abs().max())
    out["query_gradient_max_abs"] = float(gb.abs().max())
    for part in ("forward", "forward_backward"):
        fns = {fused: call(fused, part) for fused in (True, False)}
        for fn in fns.values():  # warm up: code objects, the BLAS library's choices, the allocator
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {True: [], False: []}
        for _ in range(repeats):
            for fused in (True, False):
                times[fused].append(window(fns[fused], iters))
        r = {}
        for fused, name in ((True, "fused"), (False, "unfused")):
            med = statistics.median(times[fused])
            r[name + "_us"] = {"median": round(med, 1), "min": round(min(times[fused]), 1), "max": round(max(times[fused]), 1)}
            r[name + "_peak_bytes"] = peak(fns[fused])
            if part == "forward":
                r[name + "_least_bytes_per_s"] = round(out["least_bytes_" + name] / (med * 1e-6), 0)
                r[name + "_share_of_float4_copy"] = round(out["least_bytes_" + name] / (med * 1e-6) / COPY_BYTES_PER_S, 3)
        r["unfused_over_fused_time"] = round(r["unfused_us"]["median"] / r["fused_us"]["median"], 2)
        out[part] = r
    out["note"] = "call times by device events, launch overhead and the torch matmuls included; not a kernel trace"
    return out


def main():
    args = sys.argv[1:]
    opt = {"--iters": 10, "--repeats": 7, "--hidden": 64, "--out": None}
    rows = []
    while args:
        a = args.pop(0)
        if a in opt:
            v = args.pop(0)
            opt[a] = v if a == "--out" else int(v)
        else:
            rows.append(int(a))
    if not torch.cuda.is_available():
        raise SystemExit("bench_embed.py measures on a GPU: none found")
    g = torch.Generator(device="cuda").manual_seed(1)
    res = [bench_set(key, n, content, opt["--hidden"], opt["--iters"], opt["--repeats"], g)
           for n in rows or [1024] for content in ("rollout", "all_legal") for key in SETS]
    text = "\n".join(json.dumps(r) for r in res)
    print(text)
    if opt["--out"]:
        os.makedirs(os.path.dirname(os.path.abspath(opt["--out"])), exist_ok=True)
        with open(opt["--out"], "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
