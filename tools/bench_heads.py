"""Kernel-level rate of the fused masked action heads (nmmo_amd/heads.py) on one GPU: forward with
sampling, forward with given actions and backward at the 12 nmmo head dims, the mask read in place
from flat obs rows (stride 23,987 floats), against the loop of Categoricals they replace.
Times are device events around `iters` back-to-back calls; bytes are the algorithmic ones
(logits + mask once per forward; logits + mask + gradient per backward), not measured traffic.
Under `rocprofv3 --kernel-trace --stats` the nmh_* kernel times give the same rates without the
launch overhead.

`--pointer` times the pointer heads instead (`pointer_heads`, SPEC.md §18; see `pointer_main`).

Usage (GPU box): python tools/bench_heads.py [rows] [iters] [--no-torch] [--pointer]
"""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from nmmo_amd import layout  # noqa: E402
from nmmo_amd.heads import masked_heads  # noqa: E402

OBS_ELEMS = 23987


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e-3 / iters


def torch_heads(logits, obs, dims, action=None):
    off = [0]
    for n in dims:
        off.append(off[-1] + n)
    masks = obs[:, :off[-1]] > 0
    acts, logp, ent = [], 0.0, 0.0
    for k in range(len(dims)):
        lg = logits[:, off[k]:off[k + 1]].masked_fill(~masks[:, off[k]:off[k + 1]], -1e9)
        dist = torch.distributions.Categorical(logits=lg)
        a = dist.sample() if action is None else action[:, k]
        acts.append(a)
        logp = logp + dist.log_prob(a)
        ent = ent + dist.entropy()
    return torch.stack(acts, 1), logp, ent


def pointer_main(rows, iters, key_dim=64):
    """--pointer: the 12 nmmo heads with the 8 pointer heads fused (`pointer_heads`, SPEC.md §18)
    against the unfused chain, at the two mask densities: "sparse" (what the workload produces: at
    most 8 legal market listings, ~10 entities, ~4 inventory slots, the no-op) and "all" legal."""
    from nmmo_amd.heads import pointer_heads
    from nmmo_amd.trainer import PointerMaskedAgent, pointer_logits

    dims = list(layout.ACTION_DIMS)
    total = sum(dims)
    head_set = [-1] * len(dims)
    for s, (_, names) in enumerate(PointerMaskedAgent.SETS):
        for name in names:
            head_set[layout.HEAD[name]] = s
    set_rows = [layout.PLAYER_N_OBS, layout.INVENTORY_N_OBS, layout.MARKET_N_OBS]
    n_ptr = sum(s >= 0 for s in head_set)
    n_dense = sum(n for n, s in zip(dims, head_set) if s < 0)
    off = [0]
    for n in dims:
        off.append(off[-1] + n)
    g = torch.Generator(device="cuda").manual_seed(1)
    rand = lambda *shape: torch.rand(shape, device="cuda", generator=g)  # noqa: E731
    queries = (torch.randn((rows, n_ptr, key_dim), device="cuda", generator=g) / key_dim ** 0.5).requires_grad_(True)
    keys = [torch.randn((rows, m, key_dim), device="cuda", generator=g).requires_grad_(True) for m in set_rows]
    dense = torch.randn((rows, n_dense), device="cuda", generator=g).requires_grad_(True)
    w_lp = torch.randn(rows, device="cuda", generator=g)
    leaves = [queries, dense, *keys]
    out = {"rows": rows, "iters": iters, "dims": dims, "head_set": head_set, "key_dim": key_dim}
    for density in ("sparse", "all"):
        obs = torch.zeros((rows, OBS_ELEMS), dtype=torch.float32, device="cuda")
        for k, n in enumerate(dims):
            if density == "all":
                obs[:, off[k]:off[k + 1]] = 1.0
            elif head_set[k] < 0:
                obs[:, off[k]:off[k + 1]] = (rand(rows, n) < 0.3).float()
            else:
                want = {0: 10.0, 1: 4.0, 2: 6.0}[head_set[k]]  # expected legal candidates (market: <= 8)
                legal = rand(rows, n - 1) < want / (n - 1)
                if head_set[k] == 2:
                    legal &= torch.cumsum(legal, 1) <= 8
                obs[:, off[k]:off[k + 1] - 1] = legal.float()
                obs[:, off[k + 1] - 1] = 1.0  # the no-op
        legal_keys = sum(float((obs[:, off[k]:off[k + 1] - 1] > 0).sum()) for k in range(len(dims)) if head_set[k] >= 0)
        fwd_bytes = rows * 4 * (total + n_dense + n_ptr * key_dim) + 4 * key_dim * legal_keys
        bwd_bytes = fwd_bytes + rows * 4 * (n_dense + n_ptr * key_dim + sum(set_rows) * key_dim)
        actions, _, _ = pointer_heads(queries.detach(), [k.detach() for k in keys], head_set, dense.detach(), obs, dims,
                                      seed=1)

        def backward(lp, ent):
            for t in leaves:
                t.grad = None
            (lp * w_lp + 0.01 * ent).sum().backward()

        def fused_backward():
            backward(*pointer_heads(queries, keys, head_set, dense, obs, dims, actions)[1:])

        def torch_backward():
            backward(*torch_heads(pointer_logits(queries, keys, head_set, dense, dims), obs, dims, actions.long())[1:])

        r = {"legal_keys_per_row": round(legal_keys / rows, 1), "forward_bytes_per_row": int(fwd_bytes // rows),
             "backward_bytes_per_row": int(bwd_bytes // rows)}
        with torch.no_grad():
            r["fused_sample_us"] = round(timed(lambda: pointer_heads(queries, keys, head_set, dense, obs, dims, seed=1,
                                                                     offset=3), iters) * 1e6, 2)
            r["fused_given_us"] = round(timed(lambda: pointer_heads(queries, keys, head_set, dense, obs, dims, actions),
                                              iters) * 1e6, 2)
        r["fused_forward_backward_us"] = round(timed(fused_backward, iters) * 1e6, 2)
        if "--no-torch" not in sys.argv:
            with torch.no_grad():
                r["torch_sample_us"] = round(timed(lambda: torch_heads(
                    pointer_logits(queries, keys, head_set, dense, dims), obs, dims), max(3, iters // 5)) * 1e6, 2)
            r["torch_forward_backward_us"] = round(timed(torch_backward, max(3, iters // 5)) * 1e6, 2)
        out[density] = r
    print(json.dumps(out))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rows = int(args[0]) if args else 8192
    iters = int(args[1]) if len(args) > 1 else 50
    if "--pointer" in sys.argv:
        return pointer_main(rows, iters)
    dims = list(layout.ACTION_DIMS)
    total = sum(dims)
    g = torch.Generator(device="cuda").manual_seed(1)
    obs = torch.zeros((rows, OBS_ELEMS), dtype=torch.float32, device="cuda")
    obs[:, :total] = (torch.rand((rows, total), device="cuda", generator=g) < 0.3).float()
    logits = torch.randn((rows, total), device="cuda", generator=g).requires_grad_(True)
    w_lp = torch.randn(rows, device="cuda", generator=g)
    actions, _, _ = masked_heads(logits.detach(), obs, dims, seed=1)

    def fused_backward():
        _, lp, ent = masked_heads(logits, obs, dims, actions)
        logits.grad = None
        (lp * w_lp + 0.01 * ent).sum().backward()

    def torch_backward():
        _, lp, ent = torch_heads(logits, obs, dims, actions.long())
        logits.grad = None
        (lp * w_lp + 0.01 * ent).sum().backward()

    fwd_bytes, bwd_bytes = rows * total * 8, rows * total * 12
    with torch.no_grad():
        t_sample = timed(lambda: masked_heads(logits, obs, dims, seed=1, offset=3), iters)
        t_given = timed(lambda: masked_heads(logits, obs, dims, actions), iters)
    t_fb = timed(fused_backward, iters)
    out = {"rows": rows, "dims": dims, "iters": iters,
           "forward_bytes_per_row": fwd_bytes // rows, "backward_bytes_per_row": bwd_bytes // rows,
           "fused_sample_us": round(t_sample * 1e6, 2), "fused_given_us": round(t_given * 1e6, 2),
           "fused_forward_backward_us": round(t_fb * 1e6, 2),
           "fused_sample_GBps_incl_launch": round(fwd_bytes / t_sample * 1e-9, 1)}
    if "--no-torch" not in sys.argv:
        with torch.no_grad():
            out["torch_sample_us"] = round(timed(lambda: torch_heads(logits, obs, dims), max(3, iters // 5)) * 1e6, 2)
        out["torch_forward_backward_us"] = round(timed(torch_backward, max(3, iters // 5)) * 1e6, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
