"""nml_seq_forward / nml_seq_backward (nmmo_amd/csrc/lstm.hip) at the slice edges and batch shapes
tests/test_gpu_lstm.py leaves out, called through the C entry points with every output in a guarded
buffer, against a float64 restatement of SPEC.md §17.

The sequence kernels pick 4, 2 or 1 slices of H threads from H (`slices_for`: H <= 256, <= 512,
else). Run here: H = 512, the two-slice kernel at its largest (1,024 threads, a backward LDS image of
32 KiB `dgs` + 32 KiB float64 `part`); H = 576, the one-slice kernel at its smallest (9 waves);
windows of 64 steps; NULL biases; the stored `gates`, `cs` and `dG` themselves; §17's "rows never
exchange data"; a window saturated so that every value is exact; and [T, B, 4H] offsets past 2^31
elements.

The yardstick. `spec_seq` is §17 in torch on the CPU from the kernel's own inputs: the forward step
by step, the backward in §17's closed form (no autograd). `test_spec_seq_is_torch_lstm` pins it to
`torch.nn.LSTM` with autograd in float64 on a tiny shape. `want` is `spec_seq` in float64, `E_ref`
the error of `spec_seq` in float32 against it, and the kernel passes `within` at 4 x E_ref with no
floor, each of the eight tensor kinds pooled over seeds to at least POOL elements.

Index audit of lstm.hip, read before the first full-size run (T = 17, B = 131,072, H = 256: xg,
gates and dG hold 2,281,701,376 elements; the first 16 steps end exactly on element 2^31 and the
17th, t = 16, lies past it). Every global index is formed in 64 bits:
  nml_seq_forward_kernel   row0 = blockIdx.x * kRows (int, < B <= 2^24); h0 / c0 / h_T / c_T at
                           (size_t)(row0 + r) * H + j
                           at = (size_t)t * B + row0 + r
                           xg[at * 4 * H + (size_t)g * H + j], gates[at * 4 * H + (size_t)g * H + j]
                           cs[at * H + j], y[at * H + j]; b_ih[g * H + j], b_hh[g * H + j] (< 4,096)
  rows_dot                 (w + ((size_t)(k0 + kk + u) * ldw + q * qs))[lane], ldw and qs size_t, lane
                           = s * kQ * H + j (forward, < 4H) or s * span * H + k (backward, < 4H * H
                           <= 2^22) as unsigned; v + r * ldv + k0 + kk is LDS
  nml_seq_backward_kernel  at as above; gp = gates + at * 4 * H + k, read at gp[0], gp[H] (int H <=
                           1,024), gp[2 * (size_t)H], gp[3 * (size_t)H]
                           cs[(at - B) * H + k] for t >= 1 (at >= B, B converts to size_t), cs[at * H + k]
                           dy[at * H + k]; dG[at * 4 * H + (size_t)q * H + k]
                           dh_T / dc_T / c0 / dh0 / dc0 at (size_t)(row0 + r) * H + k
  LDS                      hs[r * H + j], act[(r * 4 + g) * H + j], dgs[r * 4 * H + q * H + k],
                           part[(s * kRows + r) * H + k]: at most 16 K entries
  launch                   grid (B + kRows - 1) / kRows = 32,768 workgroups
No 32-bit product was found, so no kernel changes with this module.

Measured on an MI355X, the largest err / E_ref over the eight kinds of a case (the bound is 4):
  (8, 5, 128) 1.28 h_T    (8, 5, 192) 1.15 h_T    (2, 130, 256) 1.72 dG
  (8, 5, 512) 1.12 h_T    (3, 130, 512) 1.06 c_T  (8, 3, 512) 0.97 y
  (8, 5, 576) 1.04 cs     (8, 3, 576) 1.00 y
  (64, 5, 64) 1.12 dc0    (64, 5, 320) 1.39 y
  one NULL bias, (3, 5, H): 0.89 to 1.25
The errors themselves are 1e-7 to 5e-7 on values of unit scale: the kernels are as accurate as the
float32 restatement at every slice count, and 64 steps do not widen the gap.
"""

import functools
import math
import time

import numpy as np
import pytest
import torch

from tests.conftest import gpu_available
from tests.test_gpu_heads import within
from tests.test_gpu_lstm import assert_guards, guarded, run_cell

gpu = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not gpu_available(), reason="needs a GPU")

POOL = 2048
R = 4  # NML_ROWS
INPUTS = ("xg", "whh", "b_ih", "b_hh", "h0", "c0", "dy", "dh_T", "dc_T")
FORWARD = ("y", "h_T", "c_T", "gates", "cs")
OUTPUTS = FORWARD + ("dG", "dh0", "dc0")
# (T, B, H)
CASES = [(8, 5, 128), (8, 5, 192), (2, 130, 256),       # four slices
         (8, 5, 512), (3, 130, 512), (8, 3, 512),       # the two-slice limit
         (8, 5, 576), (8, 3, 576),                      # the first one-slice size
         (64, 5, 64), (64, 5, 320)]                     # a window eight times the trainer's horizon


# ---------------------------------------------------------------- the yardstick
def spec_seq(inputs, dtype):
    """SPEC §17 from the kernel's inputs {name: CPU tensor or None (a bias)} in `dtype`: the eight
    outputs y, h_T, c_T, gates, cs, dG, dh0, dc0 as CPU tensors of `dtype`."""
    xg, whh, b_ih, b_hh, h, c, dy, dh, dc = (None if inputs[k] is None else inputs[k].to(dtype) for k in INPUTS)
    T, B, H = dy.shape
    c0 = c
    y, gates, cs = [], [], []
    for t in range(T):
        pre = xg[t]
        if b_ih is not None:
            pre = pre + b_ih
        pre = pre + h @ whh.t()
        if b_hh is not None:
            pre = pre + b_hh
        i, f, g, o = pre.split(H, dim=1)
        i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
        c = f * c + i * g
        h = o * torch.tanh(c)
        y.append(h)
        gates.append(torch.cat([i, f, g, o], 1))
        cs.append(c)
    out = {"y": torch.stack(y), "h_T": h, "c_T": c, "gates": torch.stack(gates), "cs": torch.stack(cs)}
    dG = [None] * T
    for t in range(T - 1, -1, -1):
        i, f, g, o = out["gates"][t].split(H, dim=1)
        c_prev = out["cs"][t - 1] if t else c0
        tc = torch.tanh(out["cs"][t])
        dh = dy[t] + dh
        dc = dc + dh * o * (1 - tc * tc)
        dG[t] = torch.cat([dc * g * (i * (1 - i)), dc * c_prev * (f * (1 - f)), dc * i * (1 - g * g),
                           dh * tc * (o * (1 - o))], 1)
        dc = dc * f
        dh = dG[t] @ whh
    out.update(dG=torch.stack(dG), dh0=dh, dc0=dc)
    return out


def draw(T, B, H, seed, b_ih=True, b_hh=True):
    """The kernel's inputs as float32 CPU tensors: weights uniform(-1/sqrt(H), 1/sqrt(H)) as
    torch.nn.LSTM initialises them, unit-scale pre-activations and gradients, a state of scale 0.5."""
    rng = np.random.default_rng([seed, T, B, H])
    bound = 1 / math.sqrt(H)
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    d = {"xg": t32(rng.standard_normal((T, B, 4 * H))), "whh": t32(rng.uniform(-bound, bound, (4 * H, H))),
         "b_ih": t32(rng.uniform(-bound, bound, 4 * H)), "b_hh": t32(rng.uniform(-bound, bound, 4 * H)),
         "h0": t32(0.5 * rng.standard_normal((B, H))), "c0": t32(0.5 * rng.standard_normal((B, H))),
         "dy": t32(rng.standard_normal((T, B, H))), "dh_T": t32(rng.standard_normal((B, H))),
         "dc_T": t32(rng.standard_normal((B, H)))}
    if not b_ih:
        d["b_ih"] = None
    if not b_hh:
        d["b_hh"] = None
    return d


def test_spec_seq_is_torch_lstm():
    """`spec_seq` in float64 against torch.nn.LSTM and autograd in float64. With W_ih the identity
    (input size 4H) xg is x itself, so x's gradient is dG; the c_t of every step come from running
    the module one step at a time. The gates, which the module does not show, are pinned by their
    definition at t = 0 and by c_t = f c_{t-1} + i g, h_t = o tanh c_t at every step."""
    T, B, H = 3, 2, 4
    d = {k: v.double() for k, v in draw(T, B, H, 0).items()}
    rnn = torch.nn.LSTM(4 * H, H).double()
    rnn.load_state_dict({"weight_ih_l0": torch.eye(4 * H, dtype=torch.float64), "weight_hh_l0": d["whh"],
                         "bias_ih_l0": d["b_ih"], "bias_hh_l0": d["b_hh"]})
    x, h0, c0 = (d[k].clone().requires_grad_(True) for k in ("xg", "h0", "c0"))
    y, (h_T, c_T) = rnn(x, (h0[None], c0[None]))
    ((y * d["dy"]).sum() + (h_T[0] * d["dh_T"]).sum() + (c_T[0] * d["dc_T"]).sum()).backward()
    cs, state = [], (d["h0"][None], d["c0"][None])
    with torch.no_grad():
        for t in range(T):
            _, state = rnn(d["xg"][t:t + 1], state)
            cs.append(state[1][0])
    got = spec_seq(d, torch.float64)
    want = {"y": y.detach(), "h_T": h_T[0].detach(), "c_T": c_T[0].detach(), "cs": torch.stack(cs), "dG": x.grad,
            "dh0": h0.grad, "dc0": c0.grad}
    for k, w in want.items():
        assert got[k].shape == w.shape and float((got[k] - w).abs().max()) < 1e-13, k
    gates = got["gates"]
    assert gates.shape == (T, B, 4 * H)
    pre0 = d["xg"][0] + d["b_ih"] + d["h0"] @ d["whh"].t() + d["b_hh"]
    act0 = torch.cat([torch.sigmoid(pre0[:, :2 * H]), torch.tanh(pre0[:, 2 * H:3 * H]), torch.sigmoid(pre0[:, 3 * H:])], 1)
    assert float((gates[0] - act0).abs().max()) < 1e-15
    c = d["c0"]
    for t in range(T):
        i, f, g, o = gates[t].split(H, dim=1)
        c = f * c + i * g
        assert float((c - want["cs"][t]).abs().max()) < 1e-13 and float((o * torch.tanh(c) - want["y"][t]).abs().max()) < 1e-13
    # a NULL bias is a zero bias
    z = dict(d, b_ih=None, b_hh=torch.zeros_like(d["b_hh"]))
    a, b = spec_seq(z, torch.float64), spec_seq(dict(z, b_ih=torch.zeros_like(d["b_hh"]), b_hh=None), torch.float64)
    assert all(torch.equal(a[k], b[k]) for k in OUTPUTS)


@functools.lru_cache(maxsize=None)
def yardstick(T, B, H, seed, b_ih=True, b_hh=True):
    """(inputs, want: spec_seq in float64, ref: spec_seq in float32), computed once."""
    d = draw(T, B, H, seed, b_ih, b_hh)
    return d, spec_seq(d, torch.float64), spec_seq(d, torch.float32)


# ---------------------------------------------------------------- the kernels
def ptr(t):
    return None if t is None else t.data_ptr()


def forward(d, T, B, H):
    """nml_seq_forward on device inputs `d`: {name: (buffer, view)} of the five outputs, guarded."""
    from nmmo_amd import lstm

    out = {"y": guarded(T, B, H), "h_T": guarded(B, H), "c_T": guarded(B, H), "gates": guarded(T, B, 4 * H),
           "cs": guarded(T, B, H)}
    whh_t = d["whh"].t().contiguous()
    lstm.check(lstm.lib().nml_seq_forward(T, B, H, ptr(d["xg"]), ptr(whh_t), ptr(d["b_ih"]), ptr(d["b_hh"]), ptr(d["h0"]),
                                          ptr(d["c0"]), *[ptr(v[1]) for v in out.values()],
                                          torch.cuda.current_stream().cuda_stream), "nml_seq_forward")
    return out


def backward(d, fwd, T, B, H):
    from nmmo_amd import lstm

    out = {"dG": guarded(T, B, 4 * H), "dh0": guarded(B, H), "dc0": guarded(B, H)}
    lstm.check(lstm.lib().nml_seq_backward(T, B, H, ptr(d["dy"]), ptr(d["dh_T"]), ptr(d["dc_T"]), ptr(fwd["gates"][1]),
                                           ptr(fwd["cs"][1]), ptr(d["c0"]), ptr(d["whh"]), *[ptr(v[1]) for v in out.values()],
                                           torch.cuda.current_stream().cuda_stream), "nml_seq_backward")
    return out


def to_device(inputs):
    return {k: None if v is None else v.cuda() for k, v in inputs.items()}


def run_seq(inputs, forward_only=False):
    """Both launches on CPU inputs, backward on the gates and cs forward stored: the outputs as
    device tensors (views into their guarded buffers), guards and full coverage checked."""
    T, B, H = inputs["dy"].shape
    d = to_device(inputs)
    keep = {k: v.clone() for k, v in d.items() if v is not None}
    bufs = forward(d, T, B, H)
    if not forward_only:
        bufs |= backward(d, bufs, T, B, H)
    assert_guards(bufs)
    for k, v in keep.items():
        assert torch.equal(d[k].view(torch.int32), v.view(torch.int32)), f"{k} was written"
    return {k: v[1] for k, v in bufs.items()}


def seeds_for(T, B, H):
    """Draws until the smallest kind, a [B, H] state, pools POOL elements."""
    return range(-(-POOL // (B * H)))


def check_by_rule(T, B, H, **biases):
    """The eight outputs pooled over the case's seeds, each under `within` at 4 x E_ref; returns
    {kind: err / E_ref}."""
    pools = {k: ([], [], []) for k in OUTPUTS}
    for seed in seeds_for(T, B, H):
        d, want, ref = yardstick(T, B, H, seed, **biases)
        got = run_seq(d)
        for k in OUTPUTS:
            for dst, src in zip(pools[k], (got[k].double().cpu(), want[k], ref[k].double())):
                dst.append(src.numpy().reshape(-1))
    ratios = {}
    for k, p in pools.items():
        got, want, ref = (np.concatenate(a) for a in p)
        assert got.size >= POOL and np.abs(want).max() > 0, (k, got.size)
        err, e_ref = within(f"({T}, {B}, {H}) {biases or ''} {k}", got, want, ref)
        ratios[k] = err / e_ref
    print(f"({T}, {B}, {H}) {biases or ''}: largest err / E_ref {max(ratios.values()):.3f} ({max(ratios, key=ratios.get)})")
    return ratios


# ---------------------------------------------------------------- a. every output under the rule
@gpu
@needs_gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_all_eight_outputs_stay_within_the_float32_restatements_error(case):
    check_by_rule(*case)


# ---------------------------------------------------------------- b. NULL biases
NULL_H = [64, 320, 576]


@gpu
@needs_gpu
@pytest.mark.parametrize("H", NULL_H)
def test_null_biases_equal_zero_biases_bit_for_bit(H):
    """pre = float32(((float64(xg) + 0) + dot) + 0) is the same sum with the terms left out."""
    T, B = 3, R + 1
    d = draw(T, B, H, 11)
    zero = torch.zeros(4 * H)
    null = run_seq(dict(d, b_ih=None, b_hh=None), forward_only=True)
    zeros = run_seq(dict(d, b_ih=zero, b_hh=zero.clone()), forward_only=True)
    both = run_seq(d, forward_only=True)
    for k in FORWARD:
        assert torch.equal(null[k].view(torch.int32), zeros[k].view(torch.int32)), k
    assert not torch.equal(null["gates"], both["gates"])  # the biases do reach the gates


@gpu
@needs_gpu
@pytest.mark.parametrize("given", ["b_ih", "b_hh"])
@pytest.mark.parametrize("H", NULL_H)
def test_one_null_bias_stays_within_the_rule(H, given):
    check_by_rule(3, R + 1, H, b_ih=given == "b_ih", b_hh=given == "b_hh")


@gpu
@needs_gpu
@pytest.mark.parametrize("H", NULL_H)
def test_one_step_without_recurrence_is_nml_cell(H):
    """W_hh = 0, both biases NULL, T = 1: the dot product is 0.0 and pre = float32(float64(xg)) =
    xg, so y[0], c_T and gates[0] are nml_cell's on ga = xg[0], bit for bit."""
    B = R + 1
    d = dict(draw(1, B, H, 12), b_ih=None, b_hh=None)
    d["whh"] = torch.zeros_like(d["whh"])
    got = run_seq(d, forward_only=True)
    h, c, act = run_cell(d["xg"][0].cuda(), None, None, None, d["c0"].cuda())
    for k, want in (("y", h[None]), ("h_T", h), ("c_T", c), ("cs", c[None]), ("gates", act[None])):
        assert torch.equal(got[k].view(torch.int32), want.view(torch.int32)), k


# ---------------------------------------------------------------- c. rows do not exchange data
@gpu
@needs_gpu
@pytest.mark.parametrize("H", [64, 320, 512, 1024])
def test_rows_do_not_exchange_data(H):
    """41 rows that repeat 5 pattern rows: 5 is coprime to the 4 rows of a workgroup, so every
    pattern row meets every position of a workgroup and every set of neighbours, and the last
    workgroup holds one row. Each output row equals its pattern row's of the 5-row call, and that
    equals the call on the pattern row alone."""
    T, P, B = 3, 5, 41
    assert math.gcd(P, R) == 1 and B % R == 1
    pat = draw(T, P, H, 13)
    rows = torch.arange(B) % P

    def take(sel):
        return {k: v if k in ("whh", "b_ih", "b_hh") else v.index_select(v.dim() - 2, sel).contiguous()
                for k, v in pat.items()}

    five = run_seq(pat)
    big = run_seq(take(rows))
    for k in OUTPUTS:
        want = five[k].index_select(five[k].dim() - 2, rows.cuda())
        assert big[k].shape == want.shape and torch.equal(big[k].view(torch.int32), want.view(torch.int32)), k
    for p in range(P):
        one = run_seq(take(torch.tensor([p])))
        for k in OUTPUTS:
            want = five[k].narrow(five[k].dim() - 2, p, 1)
            assert torch.equal(one[k].view(torch.int32), want.view(torch.int32)), (k, p)


# ---------------------------------------------------------------- d. a saturated window, exact
# (i, f, g, o) signs: the four patterns of test_gpu_lstm's saturated cell test, none of which has
# f = 1 with o = 0, and a fifth that does.
SIGNS = [(1, 1, 1, 1), (-1, -1, -1, -1), (1, -1, 1, -1), (-1, 1, -1, 1), (1, 1, 1, -1)]


@gpu
@needs_gpu
@pytest.mark.parametrize("H", [64, 320])
def test_saturated_window_is_exact(H):
    """xg = +-200 and |h| <= 1, so |pre| >= 200 - sqrt(H) - 2 / sqrt(H) >= 100: §17's bound for an
    exact 0 or 1 from the sigmoid and +-1 from tanh, at every step."""
    T, B = 4, R + 1
    d = draw(T, B, H, 14)
    d["h0"] = d["h0"].clamp(-1, 1)
    d["c0"] = torch.linspace(-3, 3, B * H).view(B, H)
    reach = d["whh"].double().abs().sum(1).max() + d["b_ih"].double().abs().max() + d["b_hh"].double().abs().max()
    assert float(reach) <= math.sqrt(H) + 2 / math.sqrt(H) and 200 - float(reach) >= 100
    for s in SIGNS:
        sign = torch.tensor(s, dtype=torch.float32)
        d["xg"] = (200.0 * sign).repeat_interleave(H).repeat(T, B, 1)
        got = {k: v.cpu() for k, v in run_seq(d).items()}
        for k, v in got.items():
            assert torch.isfinite(v).all(), (s, k)
        i, f, g, o = ((sign[0] + 1) / 2, (sign[1] + 1) / 2, sign[2], (sign[3] + 1) / 2)
        act = torch.stack([i, f, g, o]).repeat_interleave(H).repeat(T, B, 1)
        assert torch.equal(got["gates"], act), s
        c = d["c0"]
        for t in range(T):
            c = f * c + i * g  # float32: both products are exact, the sum rounds once
            assert torch.equal(got["cs"][t], c), (s, t)
            if o == 0:
                assert not got["y"][t].any(), (s, t)
            else:  # o = 1: tanh(c) against torch's float32 tanh, both within a few ulps of a value below 1
                assert torch.allclose(got["y"][t], torch.tanh(c), rtol=0, atol=2.4e-7), (s, t)
        assert torch.equal(got["c_T"], c) and torch.equal(got["h_T"], got["y"][-1])
        # every derivative factor i(1 - i), f(1 - f), 1 - g^2, o(1 - o) is 0
        assert not got["dG"].any() and not got["dh0"].any(), s
        if f == 0:
            assert not got["dc0"].any(), s
        elif o == 0:  # dc passes through unchanged: dc + dh * 0 * (..) = dc, times f = 1
            assert torch.equal(got["dc0"].view(torch.int32), d["dc_T"].view(torch.int32)), s
    assert any(s[1] == 1 and s[3] == -1 for s in SIGNS)


# ---------------------------------------------------------------- e. offsets past 2^31 elements
FULL_T, FULL_B, FULL_H, K = 17, 131072, 256, 37


@gpu
@needs_gpu
def test_full_size_window_past_2_31_elements():
    """T = 17, B = 131,072, H = 256: xg, gates and dG hold 17 x 131,072 x 1,024 = 2,281,701,376
    elements, the first 16 steps end on element 2^31 and the 17th lies past it. Row r holds pattern row
    r % 37 in every input; every output row must equal the 37-row call's row r % 37, bit for bit,
    compared on the GPU in chunks. xg is freed before the backward launch.
    Measured on an MI355X: 1.2 s wall, 22.5 GiB peak device memory in use (xg, gates, y and cs
    in forward; gates, dG, cs and dy in backward)."""
    from tests.test_gpu_learner_fullsize import Guarded, tiling_holds

    T, B, H = FULL_T, FULL_B, FULL_H
    assert (T - 1) * B * 4 * H == 1 << 31 and T * B * 4 * H > 1 << 31
    GiB = 1 << 30
    need = 24 * GiB + 2 * GiB  # two [T, B, 4H] and two [T, B, H] tensors live at once (21.3 GiB), and slack
    free0, _ = torch.cuda.mem_get_info()
    if free0 < need:
        pytest.skip(f"needs {need / GiB:.0f} GiB of free device memory, {free0 / GiB:.1f} GiB are free")
    t0 = time.time()
    pat = draw(T, K, H, 15)
    ref = run_seq(pat)
    dev = to_device(pat)
    min_free = [free0]

    def note():
        torch.cuda.synchronize()
        min_free[0] = min(min_free[0], torch.cuda.mem_get_info()[0])

    def tiled(p):
        """[.., B, W] whose row r is pattern row r % K of p [.., K, W], by an expanded copy."""
        lead, W, full = p.shape[:-2], p.shape[-1], B // K
        t = torch.empty((*lead, B, W), device="cuda")
        t.narrow(-2, 0, full * K).view(*lead, full, K, W).copy_(p.unsqueeze(-3).expand(*lead, full, K, W))
        t.narrow(-2, full * K, B - full * K).copy_(p.narrow(-2, 0, B - full * K))
        return t

    def holds(got, want, name):
        if got.dim() == 2:
            got, want = got[None], want[None]
        for t in range(got.shape[0]):
            assert tiling_holds(got[t], want[t]), f"{name}: step {t}: a row differs from its pattern row's"

    from nmmo_amd import lstm

    stream = torch.cuda.current_stream().cuda_stream
    g, gy = Guarded(), Guarded()  # y is dropped before backward, with its own canaries
    d = {k: tiled(dev[k]) for k in ("xg", "h0", "c0")}
    fwd = {k: (gy if k == "y" else g).new((T, B, H) if k in ("y", "cs") else (T, B, 4 * H) if k == "gates" else (B, H))
           for k in FORWARD}
    whh_t = dev["whh"].t().contiguous()
    lstm.check(lstm.lib().nml_seq_forward(T, B, H, ptr(d["xg"]), ptr(whh_t), ptr(dev["b_ih"]), ptr(dev["b_hh"]),
                                          ptr(d["h0"]), ptr(d["c0"]), *[ptr(fwd[k]) for k in FORWARD], stream),
               "nml_seq_forward")
    note()
    g.check()
    gy.check()
    holds(d["xg"], dev["xg"], "xg after forward")
    for k in FORWARD:
        holds(fwd[k], ref[k], k)
    del d["xg"], fwd["y"], gy
    torch.cuda.empty_cache()
    for k in ("dy", "dh_T", "dc_T"):
        d[k] = tiled(dev[k])
    bwd = {k: g.new((T, B, 4 * H) if k == "dG" else (B, H)) for k in ("dG", "dh0", "dc0")}
    lstm.check(lstm.lib().nml_seq_backward(T, B, H, ptr(d["dy"]), ptr(d["dh_T"]), ptr(d["dc_T"]), ptr(fwd["gates"]),
                                           ptr(fwd["cs"]), ptr(d["c0"]), ptr(dev["whh"]), *[ptr(bwd[k]) for k in bwd],
                                           stream), "nml_seq_backward")
    note()
    g.check()
    for k in bwd:
        holds(bwd[k], ref[k], k)
    holds(fwd["gates"], ref["gates"], "gates after backward")
    note()
    del d, fwd, bwd, g
    torch.cuda.empty_cache()
    print(f"\nlstm fullsize: wall {time.time() - t0:.1f} s, peak device memory in use "
          f"{(free0 - min_free[0]) / GiB:.2f} GiB")
