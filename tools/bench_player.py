"""The fused player path (nmmo_amd/player.py, SPEC.md §21) against the unfused torch chain it
replaces, on one GPU: the same `PlayerEncoder` weights with `fused=True` and `fused=False`, the
Entity section, the AgentId and the three `*.Target` masks read from flat obs rows (stride 23,987
floats).

Content "rollout": 4-40 visible entities per row, the row's own among them, an entity legal for a
head with probability 1/4 (sparse masks). Content "all_legal": 100 entities and every entry of the
three heads legal.

Per row count (default 4,096) and content it reports, as the median and min..max over `repeats`
windows of `iters` back-to-back calls (device events; the two variants alternate window by window),
and with `torch.cuda.max_memory_allocated` over one call on top of what was allocated before it:
  forward           the own row's embedding [N, H], the pooled embedding [N, H] and the three heads'
                    logits [N, 3 x 101], under no_grad
  forward_backward  the same, forward and backward to agent_fc, my_agent_fc and the queries, the fused
                    path's small torch matmuls (`pointer_query`, the two [N, 35] linears) included
The unfused path is the reference's: one_hot, cat, agent_fc, the id match and gather, a zero row,
matmul, mean; both paths weigh only legal entries, so the gradients are the same.

Usage (GPU box): python tools/bench_player.py [rows ...] [--iters N] [--repeats N] [--hidden H] [--out FILE]
"""

import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from nmmo_amd import layout  # noqa: E402
from nmmo_amd.player import PlayerEncoder, player_logits  # noqa: E402

OBS_ELEMS = 23987
TARGETS = ("Attack.Target", "Give.Target", "GiveGold.Target")
R = layout.PLAYER_N_OBS


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
    """Flat obs rows whose Entity section, AgentId and `*.Target` masks hold `content`."""
    lay = layout.flat_layout()
    obs = torch.zeros((rows, OBS_ELEMS), dtype=torch.float32, device="cuda")
    off = lay["Entity"].offset
    ents = torch.randint(0, 160, (rows, R, 31), device="cuda", generator=g).float()
    ents[:, :, 0] = (torch.argsort(torch.rand((rows, R), device="cuda", generator=g), 1) + 1).float()  # distinct ids
    ents[:, :, 1] = torch.randint(0, 5, (rows, R), device="cuda", generator=g).float()
    if content == "rollout":  # the first k rows are filled, as the obs kernels write them
        k = torch.randint(4, 41, (rows, 1), device="cuda", generator=g)
        here = torch.arange(R, device="cuda").reshape(1, R) < k
        ents = ents * here.unsqueeze(-1)
        own = (torch.rand((rows,), device="cuda", generator=g) * k[:, 0]).long()
    else:
        here = torch.ones((rows, R), dtype=torch.bool, device="cuda")
        own = torch.randint(0, R, (rows,), device="cuda", generator=g)
    obs[:, off:off + 31 * R] = ents.reshape(rows, -1)
    obs[:, lay["AgentId"].offset] = ents[torch.arange(rows, device="cuda"), own, 0]
    offs = [lay[f"ActionTargets.{h}"].offset for h in TARGETS]
    for o in offs:
        legal = here if content == "all_legal" else here & (torch.rand((rows, R), device="cuda", generator=g) < 0.25)
        obs[:, o:o + R] = legal.float()
        obs[:, o + R] = 1.0  # the no-op
    return obs, obs[:, off:off + 31 * R], obs[:, lay["AgentId"].offset], offs


def bench_rows(rows, content, hidden, iters, repeats):
    g = torch.Generator(device="cuda").manual_seed(1)
    obs, ents, ids, offs = make_obs(rows, content, g)
    torch.manual_seed(2)
    enc = {True: PlayerEncoder(hidden, hidden, fused=True).cuda(), False: PlayerEncoder(hidden, hidden).cuda()}
    enc[False].load_state_dict(enc[True].state_dict())
    q0 = torch.randn((rows, 3, hidden), device="cuda", generator=g) / hidden
    w_pool = torch.randn((rows, hidden), device="cuda", generator=g)
    w_mine = torch.randn((rows, hidden), device="cuda", generator=g)
    w_lg = torch.cat([obs[:, o:o + R + 1] for o in offs], 1).clone()  # 0 where illegal and for the no-op
    w_lg[:, R::R + 1] = 0
    w_lg = w_lg * torch.randn(w_lg.shape, device="cuda", generator=g)

    def path(fused, q, m=None, ents=ents, ids=ids, rows_=obs):
        m = m or enc[fused]
        if fused:
            return m.my_agent(ents, ids), m.pooled(ents), player_logits(ents, m.pointer_query(q), rows_, offs)
        feats = m.features(ents)  # made once, as in the reference's forward
        col = feats[..., 0]
        match = (col == ids.reshape(-1, 1).to(col.dtype)) & (col != 0)
        idx = torch.where(match.any(1), match.int().argmax(1), torch.zeros_like(match.sum(1)))
        mine = torch.relu(m.my_agent_fc(feats[torch.arange(rows, device=feats.device), idx]))
        emb = m.agent_fc(feats)
        padded = torch.cat([emb, emb.new_zeros(rows, 1, hidden)], 1)
        lg = torch.cat([torch.matmul(padded, q[:, i].to(emb.dtype).unsqueeze(-1)).squeeze(-1) for i in range(3)], 1)
        return mine, emb.mean(1), lg

    def call(fused, part):
        def fn():
            if part == "forward":
                with torch.no_grad():
                    return path(fused, q0)
            for p in enc[fused].parameters():
                p.grad = None
            q = q0.clone().requires_grad_(True)
            mine, pooled, lg = path(fused, q)
            ((mine * w_mine).sum() + (pooled * w_pool).sum() + (lg * w_lg).sum()).backward()
            return q.grad
        return fn

    out = {"rows": rows, "content": content, "hidden": hidden, "iters": iters, "repeats": repeats,
           "entity_embedding_bytes_per_row_unfused": R * hidden * 4, "entity_section_bytes_per_row": R * 31 * 4,
           "legal_candidates_per_row": round(float((w_lg != 0).sum()) / rows, 2)}
    legal = w_lg != 0
    with torch.no_grad():
        a, b = path(True, q0), path(False, q0)
        out["my_agent_max_abs_difference"] = float((a[0] - b[0]).abs().max())
        out["pooled_max_abs_difference"] = float((a[1] - b[1]).abs().max())
        out["legal_logits_max_abs_difference"] = float(((a[2] - b[2]) * legal).abs().max())
        out["legal_logits_max_abs"] = float((b[2] * legal).abs().max())
    ga, gb = call(True, "forward_backward")(), call(False, "forward_backward")()
    out["query_gradient_max_abs_difference"] = float((ga - gb).abs().max())
    out["query_gradient_max_abs"] = float(gb.abs().max())
    # both against the unfused chain in float64
    enc64 = PlayerEncoder(hidden, hidden).cuda().double()
    enc64.load_state_dict(enc[True].state_dict())
    obs64 = obs.double()
    e64 = obs64[:, ents.storage_offset() % OBS_ELEMS:][:, :31 * R]
    q64 = q0.double().requires_grad_(True)
    mine, pooled, lg = path(False, q64, enc64, e64, obs64[:, ids.storage_offset() % OBS_ELEMS])
    ((mine * w_mine).sum() + (pooled * w_pool).sum() + (lg * w_lg).sum()).backward()
    for name, m in (("fused", enc[True]), ("unfused", enc[False])):
        out[f"agent_fc_weight_gradient_max_error_{name}_vs_float64"] = float(
            (m.agent_fc.weight.grad - enc64.agent_fc.weight.grad).abs().max())
    out["agent_fc_weight_gradient_max_abs"] = float(enc64.agent_fc.weight.grad.abs().max())
    out["query_gradient_max_error_fused_vs_float64"] = float((ga - q64.grad).abs().max())
    out["query_gradient_max_error_unfused_vs_float64"] = float((gb - q64.grad).abs().max())
    del enc64, obs64, e64, q64, mine, pooled, lg
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
            r[name + "_us"] = {"median": round(statistics.median(times[fused]), 1),
                               "min": round(min(times[fused]), 1), "max": round(max(times[fused]), 1)}
            r[name + "_peak_bytes"] = peak(fns[fused])
        r["unfused_over_fused_time"] = round(r["unfused_us"]["median"] / r["fused_us"]["median"], 2)
        r["unfused_over_fused_peak"] = round(r["unfused_peak_bytes"] / max(1, r["fused_peak_bytes"]), 2)
        out[part] = r
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
        raise SystemExit("bench_player.py measures on a GPU: none found")
    res = [bench_rows(n, content, opt["--hidden"], opt["--iters"], opt["--repeats"])
           for n in rows or [4096] for content in ("rollout", "all_legal")]
    text = "\n".join(json.dumps(r) for r in res)
    print(text)
    if opt["--out"]:
        os.makedirs(os.path.dirname(os.path.abspath(opt["--out"])), exist_ok=True)
        with open(opt["--out"], "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
