"""Kernel-level rate of the fused masked action heads (nmmo_amd/heads.py) on one GPU: forward with
sampling, forward with given actions and backward at the 12 nmmo head dims, the mask read in place
from flat obs rows (stride 23,987 floats), against the loop of Categoricals they replace.
Times are device events around `iters` back-to-back calls; bytes are the algorithmic ones
(logits + mask once per forward; logits + mask + gradient per backward), not measured traffic.
Under `rocprofv3 --kernel-trace --stats` the nmh_* kernel times give the same rates without the
launch overhead.

Usage (GPU box): python tools/bench_heads.py [rows] [iters] [--no-torch]
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


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rows = int(args[0]) if args else 8192
    iters = int(args[1]) if len(args) > 1 else 50
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
