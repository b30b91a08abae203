"""The fused item path (nmmo_amd/item.py, SPEC.md §20) against the unfused torch chain it replaces,
on one GPU: the same `ItemEncoder` weights with `fused=True` and `fused=False`, the Inventory and
Market sections read from flat obs rows (stride 23,987 floats).

Content "rollout": 0-8 listings and about 4 inventory items per row, a listing or item legal for a
head with probability 1/2 (sparse masks). Content "all_legal": every one of the 1,024 + 12 slots
holds an item and every entry of the five heads is legal.

Per row count (default 1,024 and 4,096) and content it reports, as the median and min..max over
`repeats` windows of `iters` back-to-back calls (device events; the two variants alternate window
by window), and with `torch.cuda.max_memory_allocated` over one call on top of what was allocated
before it:
  pooled            (a) the pooled market embedding [N, H], forward under no_grad
  logits            (b) the five item heads' logits (4 x 13 + 1,025 per row), forward under no_grad
  forward_backward  (c) (a) + (b) forward and backward to fc and the queries, the fused path's
                    small torch matmuls (`pointer_query`, the [N, 32] linear) included
and the `nmh_item_features` sums call alone over the Market sections as bytes read per second, next
to the 6.29 TB/s float4 copy DESIGN §3.12 quotes. The unfused logits are the reference's: embed,
pad a zero row, matmul; for (c) both paths weigh only legal entries, so the gradients are the same.

Usage (GPU box): python tools/bench_item.py [rows ...] [--iters N] [--repeats N] [--hidden H] [--out FILE]
"""

import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from nmmo_amd import layout  # noqa: E402
from nmmo_amd.item import ItemEncoder, item_logits, item_sums  # noqa: E402

OBS_ELEMS = 23987
COPY_BYTES_PER_S = 6.29e12  # the float4 copy kernel on this GPU
INV_HEADS = ("Destroy.InventoryItem", "Give.InventoryItem", "Sell.InventoryItem", "Use.InventoryItem")


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
    """Flat obs rows whose Inventory and Market sections and item-head masks hold `content`."""
    lay = layout.flat_layout()
    obs = torch.zeros((rows, OBS_ELEMS), dtype=torch.float32, device="cuda")
    sets = []
    for name, heads_ in (("Inventory", INV_HEADS), ("Market", ("Buy.MarketItem",))):
        R, off = lay[name].shape[0], lay[name].offset
        items = torch.randint(0, 100, (rows, R, 16), device="cuda", generator=g).float()
        items[:, :, 0] = torch.randint(1, 30000, (rows, R), device="cuda", generator=g).float()
        items[:, :, 1] = torch.randint(1, 18, (rows, R), device="cuda", generator=g).float()
        items[:, :, 14] = torch.randint(0, 2, (rows, R), device="cuda", generator=g).float()
        if content == "rollout":  # the first k slots are filled, as the obs kernels write them
            k = torch.randint(0, 9, (rows, 1), device="cuda", generator=g)
            here = torch.arange(R, device="cuda").reshape(1, R) < k
            items = items * here.unsqueeze(-1)
        else:
            here = torch.ones((rows, R), dtype=torch.bool, device="cuda")
        obs[:, off:off + 16 * R] = items.reshape(rows, -1)
        offs = [lay[f"ActionTargets.{h}"].offset for h in heads_]
        for o in offs:
            legal = here if content == "all_legal" else here & (torch.rand((rows, R), device="cuda", generator=g) < 0.5)
            obs[:, o:o + R] = legal.float()
            obs[:, o + R] = 1.0  # the no-op
        sets.append((obs[:, off:off + 16 * R], R, offs))
    return obs, sets


def bench_rows(rows, content, hidden, iters, repeats):
    g = torch.Generator(device="cuda").manual_seed(1)
    obs, sets = make_obs(rows, content, g)
    market = sets[1][0]
    torch.manual_seed(2)
    enc = {True: ItemEncoder(hidden, fused=True).cuda(), False: ItemEncoder(hidden, fused=False).cuda()}
    enc[False].load_state_dict(enc[True].state_dict())
    q0 = torch.randn((rows, 5, hidden), device="cuda", generator=g) / hidden ** 0.5
    w_pool = torch.randn((rows, hidden), device="cuda", generator=g)
    # weights of the heads' entries, 0 where illegal (and for the no-op, a constant): [N, 4 * 13], [N, 1025]
    w_lg = []
    for _, R, offs in sets:
        w = torch.cat([obs[:, o:o + R + 1] for o in offs], 1).clone()
        w[:, R::R + 1] = 0
        w_lg.append(w * torch.randn(w.shape, device="cuda", generator=g))

    def pooled(fused, m=None, mk=market):
        return (m or enc[fused]).pooled(mk)

    def logits(fused, q, m=None, sets=sets):
        m, out, p = m or enc[fused], [], 0
        if fused:
            pq = m.pointer_query(q)
            for items, R, offs in sets:
                out.append(item_logits(items, pq[:, p:p + len(offs)], obs, offs))
                p += len(offs)
            return out
        for items, R, offs in sets:
            emb = m.embed(items)
            padded = torch.cat([emb, emb.new_zeros(rows, 1, hidden)], 1)
            out.append(torch.cat([torch.matmul(padded, q[:, p + i].to(emb.dtype).unsqueeze(-1)).squeeze(-1)
                                  for i in range(len(offs))], 1))
            p += len(offs)
        return out

    def call(fused, part):
        def fn():
            if part != "forward_backward":
                with torch.no_grad():
                    return pooled(fused) if part == "pooled" else logits(fused, q0)
            for p in enc[fused].parameters():
                p.grad = None
            q = q0.clone().requires_grad_(True)
            loss = (pooled(fused) * w_pool).sum()
            for lg, w in zip(logits(fused, q), w_lg):
                loss = loss + (lg * w).sum()
            loss.backward()
            return q.grad
        return fn

    out = {"rows": rows, "content": content, "hidden": hidden, "iters": iters, "repeats": repeats,
           "market_embedding_bytes_per_row_unfused": 1024 * hidden * 4, "market_section_bytes_per_row": 1024 * 64,
           "legal_candidates_per_row": round(sum(float((w != 0).sum()) for w in w_lg) / rows, 2)}
    with torch.no_grad():
        out["pooled_max_abs_difference"] = float((pooled(True) - pooled(False)).abs().max())
        legal = [w != 0 for w in w_lg]
        out["legal_logits_max_abs_difference"] = max(
            float(((a - b) * l).abs().max()) for a, b, l in zip(logits(True, q0), logits(False, q0), legal))
    ga, gb = call(True, "forward_backward")(), call(False, "forward_backward")()
    out["query_gradient_max_abs_difference"] = float((ga - gb).abs().max())
    out["query_gradient_max_abs"] = float(gb.abs().max())
    out["fc_weight_gradient_max_abs_difference"] = float((enc[True].fc.weight.grad - enc[False].fc.weight.grad).abs().max())
    out["fc_weight_gradient_max_abs"] = float(enc[False].fc.weight.grad.abs().max())
    # both against the unfused chain in float64
    enc64 = ItemEncoder(hidden).cuda().double()
    enc64.load_state_dict(enc[True].state_dict())
    obs64 = obs.double()
    sets64 = [(obs64[:, items.storage_offset() % OBS_ELEMS:][:, :16 * R], R, offs) for items, R, offs in sets]
    q64 = q0.double().requires_grad_(True)
    loss = (pooled(False, enc64, sets64[1][0]) * w_pool).sum()
    for lg, w in zip(logits(False, q64, enc64, sets64), w_lg):
        loss = loss + (lg * w).sum()
    loss.backward()
    for name, m in (("fused", enc[True]), ("unfused", enc[False])):
        out[f"fc_weight_gradient_max_error_{name}_vs_float64"] = float((m.fc.weight.grad - enc64.fc.weight.grad).abs().max())
    out["query_gradient_max_error_fused_vs_float64"] = float((ga - q64.grad).abs().max())
    out["query_gradient_max_error_unfused_vs_float64"] = float((gb - q64.grad).abs().max())
    del enc64, obs64, sets64, q64, loss
    for part in ("pooled", "logits", "forward_backward"):
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
    sums = [window(lambda: item_sums(market), iters) for _ in range(repeats + 1)][1:]
    med = statistics.median(sums)
    out["sums_call"] = {"us": {"median": round(med, 1), "min": round(min(sums), 1), "max": round(max(sums), 1)},
                        "bytes_read": rows * 1024 * 64, "bytes_per_s": round(rows * 1024 * 64 / (med * 1e-6), 0),
                        "share_of_float4_copy": round(rows * 1024 * 64 / (med * 1e-6) / COPY_BYTES_PER_S, 3),
                        "note": "call time by device events, launch overhead included; not a kernel trace"}
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
        raise SystemExit("bench_item.py measures on a GPU: none found")
    res = [bench_rows(n, content, opt["--hidden"], opt["--iters"], opt["--repeats"])
           for n in rows or [1024, 4096] for content in ("rollout", "all_legal")]
    text = "\n".join(json.dumps(r) for r in res)
    print(text)
    if opt["--out"]:
        os.makedirs(os.path.dirname(os.path.abspath(opt["--out"])), exist_ok=True)
        with open(opt["--out"], "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
