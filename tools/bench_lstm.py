"""Rate of the fused LSTM recurrence (nmmo_amd/lstm.py) on one GPU against torch.nn.LSTM on the same
card in the same process, at the shapes of the device train loop with the start-kit policy
(input = hidden = 256, one layer):

  train     one bptt window, T = 8 steps of B = 128 rows, forward + backward (grad mode:
            nml_seq_forward / nml_seq_backward, one launch each, plus the GEMMs over T * B rows)
  eval      one step over B = 8,192 and B = 131,072 agent slots under no_grad (addmm_ + nml_cell,
            the state updated in place)

Variants, alternated, `reps` repetitions each, one JSON line per (repetition, variant):
  fused     lstm.LSTM
  torch     torch.nn.LSTM with torch.backends.cudnn.flags(enabled=False): torch's own fused cell
  miopen    torch.nn.LSTM as it comes (MIOpen); left out with --no-miopen, and reported as an
            error string if it does not run
Times are device events around `iters` back-to-back calls, so they include launch overhead. For
kernel times run one variant alone under the profiler, in a run of its own:

  rocprofv3 --kernel-trace --stats -- python tools/bench_lstm.py --only fused --reps 1

Usage (GPU box): python tools/bench_lstm.py [--iters N] [--reps N] [--only VARIANT] [--no-miopen]
"""

import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from nmmo_amd import lstm  # noqa: E402

H = 256
TRAIN = (8, 128)
EVAL_ROWS = (8192, 131072)


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
    return round(t0.elapsed_time(t1) * 1e3 / iters, 2)  # us


def option(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def measure(variant, rnn, iters):
    """{shape: us per call} for one variant; `rnn` holds the shared weights."""
    fused = variant == "fused"
    ctx = torch.backends.cudnn.flags(enabled=False) if variant == "torch" else contextlib.nullcontext()
    g = torch.Generator(device="cuda").manual_seed(1)
    out = {}
    with ctx:
        T, B = TRAIN
        x = torch.randn((T, B, H), device="cuda", generator=g).requires_grad_(True)
        w = torch.randn((T, B, H), device="cuda", generator=g)

        def train_step():
            y, (h, c) = rnn(x, None)
            x.grad = None
            rnn.zero_grad(set_to_none=True)
            ((y * w).sum() + h.sum() + c.sum()).backward()

        def forward_only():
            rnn(x, None)

        out[f"train_T{T}_B{B}_forward_us"] = timed(forward_only, iters)
        out[f"train_T{T}_B{B}_forward_backward_us"] = timed(train_step, iters)
        with torch.no_grad():
            for rows in EVAL_ROWS:
                xe = torch.randn((1, rows, H), device="cuda", generator=g)
                state = [torch.zeros((1, rows, H), device="cuda"), torch.zeros((1, rows, H), device="cuda")]

                def eval_step():
                    if fused:
                        rnn(xe, tuple(state), out=tuple(state))
                    else:
                        _, (state[0], state[1]) = rnn(xe, tuple(state))

                out[f"eval_B{rows}_us"] = timed(eval_step, max(5, iters // 4) if rows > 8192 else iters)
    return out


def main():
    iters, reps = option("--iters", 50), option("--reps", 2)
    variants = ["fused", "torch"] + ([] if "--no-miopen" in sys.argv else ["miopen"])
    if "--only" in sys.argv:
        variants = [sys.argv[sys.argv.index("--only") + 1]]
    torch.manual_seed(1)
    theirs = torch.nn.LSTM(H, H).cuda()
    ours = lstm.LSTM(H, H).cuda()
    ours.load_state_dict(theirs.state_dict())
    for rep in range(reps):
        for variant in variants:
            line = {"variant": variant, "rep": rep, "hidden": H, "iters": iters}
            try:
                line.update(measure(variant, ours if variant == "fused" else theirs, iters))
            except RuntimeError as e:
                if variant != "miopen":
                    raise
                line["error"] = str(e).splitlines()[0][:200]  # MIOpen without its kernel database
                print(json.dumps(line), flush=True)
                return  # nothing more runs on the card after an error
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
