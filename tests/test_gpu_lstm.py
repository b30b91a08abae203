"""The fused LSTM recurrence (nmmo_amd/lstm.py, csrc/lstm.hip) on MI355X against SPEC.md §17.

The checker is `torch.nn.LSTM` on the CPU in float64 with the same weights. `E_ref` is the error
against it of `torch.nn.LSTM` on the CPU in float32, and the fused result must stay within
4 x E_ref with no floor (`tests/test_gpu_heads.py::within`). A rule without a floor
needs enough elements per compared tensor (E_ref of four numbers can be lucky), so every tensor
kind is pooled over seeds until the pool holds at least POOL elements, and both errors are the
maximum over the pool. No test runs torch.nn.LSTM on the GPU.

Shapes: H 64 (one wave), 256 (the reference's), 320 (not a power of two), 1024 (the limit: the
largest workgroup and LDS image); B 1, ROWS - 1, ROWS + 1, 130 around the sequence kernels' rows per
workgroup; T 1 and 8; input size 24 != H; one and two layers; state given and None.
"""

import functools

import numpy as np
import pytest
import torch

from tests.conftest import gpu_available
from tests.test_gpu_heads import within

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

I = 24
POOL = 2048
R = 4  # lstm.ROWS, asserted below
# (T, B, H, num_layers, state given)
CASES = [(1, 1, 64, 1, True), (8, R - 1, 64, 2, False), (8, R + 1, 64, 1, True), (8, 130, 64, 2, True),
         (1, 130, 256, 1, False), (8, R + 1, 256, 1, True), (8, R - 1, 320, 2, True), (1, R + 1, 320, 1, False),
         (8, 130, 320, 1, True), (2, R + 1, 1024, 1, True),
         # the slice edges of tests/test_gpu_lstm_shapes.py through the module: two slices at their largest H,
         # one slice at its smallest, four slices at an H that is not a power of two
         (8, 5, 512, 1, True), (8, 3, 576, 2, True), (8, 5, 192, 1, False)]
PARAMS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def test_rows_constant():
    from nmmo_amd import lstm

    assert lstm.ROWS == R


# ---------------------------------------------------------------- the yardstick
@functools.lru_cache(maxsize=None)
def reference(case, seed):
    """Inputs, weights and torch.nn.LSTM's results on the CPU, in float64 (`want`) and float32
    (`ref`), for one draw. The loss is a fixed weighted sum of y, h_T and c_T."""
    T, B, H, L, given = case
    rng = np.random.default_rng([seed, T, B, H, L])
    inp = {"x": rng.standard_normal((T, B, I)), "h0": 0.5 * rng.standard_normal((L, B, H)),
           "c0": 0.5 * rng.standard_normal((L, B, H))}
    wts = {"y": rng.standard_normal((T, B, H)), "h_T": rng.standard_normal((L, B, H)),
           "c_T": rng.standard_normal((L, B, H))}
    bound = 1 / np.sqrt(H)
    sd = {}
    for k in range(L):
        for name, shape in zip(PARAMS, ((4 * H, I if k == 0 else H), (4 * H, H), (4 * H,), (4 * H,))):
            sd[f"{name}_l{k}"] = rng.uniform(-bound, bound, shape).astype(np.float32)
    inp = {k: v.astype(np.float32) for k, v in inp.items()}
    out = {"inp": inp, "wts": wts, "sd": sd}
    for key, dtype in (("want", torch.float64), ("ref", torch.float32)):
        rnn = torch.nn.LSTM(I, H, L).to(dtype)
        rnn.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in sd.items()})
        out[key] = run(rnn, inp, wts, given, dtype, "cpu")
    return out


def run(rnn, inp, wts, given, dtype, device, grad=True, **kw):
    """One forward (and backward) of `rnn`: {kind: float64 numpy array}."""
    t = {k: torch.from_numpy(v).to(device=device, dtype=dtype).requires_grad_(grad) for k, v in inp.items()}
    w = {k: torch.from_numpy(v).to(device=device, dtype=dtype) for k, v in wts.items()}
    state = (t["h0"], t["c0"]) if given else None
    with torch.set_grad_enabled(grad):
        y, (h_T, c_T) = rnn(t["x"], state, **kw)
    res = {"y": y, "h_T": h_T, "c_T": c_T}
    if grad:
        ((y * w["y"]).sum() + (h_T * w["h_T"]).sum() + (c_T * w["c_T"]).sum()).backward()
        res["dx"] = t["x"].grad
        if given:
            res["dh0"], res["dc0"] = t["h0"].grad, t["c0"].grad
        for k, p in rnn.named_parameters():
            res["d" + k] = p.grad
    return {k: v.detach().double().cpu().numpy() for k, v in res.items()}


def fused_module(case, seed):
    from nmmo_amd import lstm

    T, B, H, L, given = case
    rnn = lstm.LSTM(I, H, L)
    rnn.load_state_dict({k: torch.from_numpy(v) for k, v in reference(case, seed)["sd"].items()})
    return rnn.cuda()


def seeds_for(case):
    """Draws until the smallest compared tensor kind (the state [L, B, H], one layer's bias
    gradient [4H], or x's gradient [T, B, I]) pools POOL elements."""
    T, B, H, L, given = case
    return range(-(-POOL // min(L * B * H, 4 * H, T * B * I)))


def check_pooled(case, got_of, kinds=None):
    """`got_of(seed)` -> {kind: array}; each kind pooled over the case's seeds, under the rule."""
    pools = {}
    for seed in seeds_for(case):
        o = reference(case, seed)
        got = got_of(seed)
        for kind in (kinds or o["want"]):
            p = pools.setdefault(kind, ([], [], []))
            for dst, src in zip(p, (got, o["want"], o["ref"])):
                dst.append(src[kind].reshape(-1))
    for kind, p in pools.items():
        got, want, ref = (np.concatenate(a) for a in p)
        assert got.size >= POOL, (kind, got.size)
        within(f"{case} {kind}", got, want, ref)
    return pools


# ---------------------------------------------------------------- 1. the sequence path (grad)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_sequence_path_forward_and_gradients(case):
    """nml_seq_forward / nml_seq_backward through `lstm.LSTM` with grad enabled: y, h_T, c_T, the
    gradients of x, h0, c0 and of the four parameters of every layer."""
    T, B, H, L, given = case

    def got_of(seed):
        o = reference(case, seed)
        return run(fused_module(case, seed), o["inp"], o["wts"], given, torch.float32, "cuda")

    pools = check_pooled(case, got_of)
    want = {"y", "h_T", "c_T", "dx"} | {f"d{p}_l{k}" for p in PARAMS for k in range(L)}
    assert set(pools) == want | ({"dh0", "dc0"} if given else set())


# ---------------------------------------------------------------- 2. the step path (no grad)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_step_path_matches_the_checker(case):
    """addmm_ + nml_cell per step under torch.no_grad(), on the inputs of the grad path."""
    T, B, H, L, given = case

    def got_of(seed):
        o = reference(case, seed)
        return run(fused_module(case, seed), o["inp"], o["wts"], given, torch.float32, "cuda", grad=False)

    check_pooled(case, got_of, kinds=("y", "h_T", "c_T"))


@pytest.mark.parametrize("case", [CASES[3], CASES[4]], ids=str)
def test_out_updates_the_state_in_place(case):
    T, B, H, L, given = case
    o = reference(case, 0)
    rnn = fused_module(case, 0)
    x, h0, c0 = (torch.from_numpy(o["inp"][k]).cuda() for k in ("x", "h0", "c0"))
    with torch.no_grad():
        y1, (h1, c1) = rnn(x, (h0, c0))
        assert h1.data_ptr() != h0.data_ptr() and torch.equal(h0.cpu(), torch.from_numpy(o["inp"]["h0"]))
        h, c = h0.clone(), c0.clone()
        ptrs = h.data_ptr(), c.data_ptr()
        y2, (h2, c2) = rnn(x, (h, c), out=(h, c))
        assert h2 is h and c2 is c and (h.data_ptr(), c.data_ptr()) == ptrs
        assert torch.equal(h, h1) and torch.equal(c, c1) and torch.equal(y2, y1)
        assert (y2.data_ptr() == h[L - 1].data_ptr()) == (T == 1)
        # a separate out= leaves the given state alone
        ho, co = torch.empty_like(h0), torch.empty_like(c0)
        rnn(x, (h0, c0), out=(ho, co))
        assert torch.equal(ho, h1) and torch.equal(co, c1)
        assert torch.equal(c0.cpu(), torch.from_numpy(o["inp"]["c0"]))
    with pytest.raises(ValueError):
        rnn(x, (h0, c0), out=(h0, c0))  # grad mode: the state is not written in place


# ---------------------------------------------------------------- 3. nml_cell itself
def cell_inputs(B, H, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: (scale * torch.randn(*s, generator=g)).cuda()  # noqa: E731
    return dict(ga=mk(B, 4 * H), gb=mk(B, 4 * H), b_ih=mk(4 * H), b_hh=mk(4 * H), c_prev=mk(B, H))


def run_cell(ga, gb, b_ih, b_hh, c_prev, gates=True):
    from nmmo_amd import lstm

    h, c = torch.empty_like(c_prev), torch.empty_like(c_prev)
    act = torch.empty_like(ga) if gates else None
    lstm.cell(ga, gb, b_ih, b_hh, c_prev, h, c, act)
    return h, c, act


@pytest.mark.parametrize("case", [(1, 1, 64, 1, True), (1, 130, 256, 1, True), (1, R + 1, 320, 1, True)], ids=str)
def test_cell_with_two_addends_matches_the_checker(case):
    """x W_ih^T and h W_hh^T as nml_cell's two addends, both biases: one step of torch.nn.LSTM."""
    T, B, H, L, given = case

    def got_of(seed):
        o = reference(case, seed)
        x, h0, c0 = (torch.from_numpy(o["inp"][k]).cuda() for k in ("x", "h0", "c0"))
        w_ih, w_hh, b_ih, b_hh = (torch.from_numpy(o["sd"][f"{p}_l0"]).cuda() for p in PARAMS)
        h, c, _ = run_cell(x[0] @ w_ih.t(), h0[0] @ w_hh.t(), b_ih, b_hh, c0[0])
        return {"h_T": h.double().cpu().numpy()[None], "c_T": c.double().cpu().numpy()[None]}

    check_pooled(case, got_of, kinds=("h_T", "c_T"))


@pytest.mark.parametrize("B,H", [(1, 64), (R + 1, 320), (130, 256)])
def test_cell_aliased_call_equals_out_of_place(B, H):
    from nmmo_amd import lstm

    a = cell_inputs(B, H, seed=1)
    h, c, act = run_cell(**a)
    c_io, ga_io, h_io = a["c_prev"].clone(), a["ga"].clone(), torch.empty(B, H, device="cuda")
    lstm.cell(ga_io, a["gb"], a["b_ih"], a["b_hh"], c_io, h_io, c_io, ga_io)  # c and the gates in place
    assert torch.equal(h_io, h) and torch.equal(c_io, c) and torch.equal(ga_io, act)
    h2, c2, none = run_cell(**a, gates=False)
    assert none is None and torch.equal(h2, h) and torch.equal(c2, c)


@pytest.mark.parametrize("B,H", [(R + 1, 64), (130, 320)])
def test_cell_one_addend_without_biases_equals_two_addends_on_the_same_sums(B, H):
    a = cell_inputs(B, H, seed=2)
    two = run_cell(a["ga"], a["gb"], None, None, a["c_prev"])
    one = run_cell(a["ga"] + a["gb"], None, None, None, a["c_prev"])
    for x, y in zip(one, two):
        assert torch.equal(x, y)
    # and the four terms are added left to right: ga + b_ih + gb + b_hh
    full = run_cell(**a)
    summed = run_cell(((a["ga"] + a["b_ih"]) + a["gb"]) + a["b_hh"], None, None, None, a["c_prev"])
    for x, y in zip(summed, full):
        assert torch.equal(x, y)


def test_cell_scalar_path_equals_vector_path():
    """Buffers that are not 16-byte aligned take the dword kernel: the same bits."""
    B, H = R + 1, 64
    a = cell_inputs(B, H, seed=3)
    want = run_cell(**a)

    def off(t):  # the same values at an address that is 4 mod 16
        buf = torch.empty(t.numel() + 1, device="cuda")
        assert buf.data_ptr() % 16 == 0
        v = buf[1:].view(t.shape)
        v.copy_(t)
        return v

    got = run_cell(**{k: off(v) for k, v in a.items()})
    for x, y in zip(got, want):
        assert torch.equal(x, y)


def test_cell_saturated_gates_are_exact_and_finite():
    """|pre| = 100: sigmoid gives exactly 0 or 1, tanh exactly +-1, never a NaN."""
    B, H = 2, 64
    signs = torch.tensor([[1.0, 1.0, 1.0, 1.0], [-1.0, -1.0, -1.0, -1.0], [1.0, -1.0, 1.0, -1.0],
                          [-1.0, 1.0, -1.0, 1.0]])
    c_prev = torch.linspace(-3, 3, B * H).view(B, H).cuda()
    for s in signs:
        ga = (100.0 * s).repeat_interleave(H).repeat(B, 1).cuda()
        h, c, act = run_cell(ga, None, None, None, c_prev)
        assert torch.isfinite(h).all() and torch.isfinite(c).all()
        want = ((s + 1) / 2).clone()
        want[2] = s[2]  # g is a tanh
        assert torch.equal(act.cpu(), want.repeat_interleave(H).repeat(B, 1))
        i, f, g, o = want.tolist()
        assert torch.equal(c, f * c_prev + i * g)
        # o is exactly 0 or 1; tanh(c) against torch's float32 tanh, both within a few ulps of a value below 1
        assert torch.equal(h, torch.zeros_like(h)) if o == 0 else torch.allclose(h, torch.tanh(c), rtol=0, atol=2.4e-7)


# ---------------------------------------------------------------- 4. determinism, stream, bounds
def test_same_inputs_give_bit_identical_results():
    case = CASES[3]
    o = reference(case, 0)
    rnn = fused_module(case, 0)
    a, b = (run(rnn_, o["inp"], o["wts"], True, torch.float32, "cuda") for rnn_ in (rnn, fused_module(case, 0)))
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_runs_on_the_current_stream():
    case = CASES[5]
    o = reference(case, 0)
    a = run(fused_module(case, 0), o["inp"], o["wts"], True, torch.float32, "cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = run(fused_module(case, 0), o["inp"], o["wts"], True, torch.float32, "cuda")
        c = run(fused_module(case, 0), o["inp"], o["wts"], True, torch.float32, "cuda", grad=False)
    side.synchronize()
    a_nograd = run(fused_module(case, 0), o["inp"], o["wts"], True, torch.float32, "cuda", grad=False)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    for k in c:
        assert np.array_equal(a_nograd[k], c[k]), k


G = 64  # guard elements on both sides of every output


def guarded(*shape):
    n = int(np.prod(shape))
    buf = torch.full((G + n + G,), 12345.0, dtype=torch.float32, device="cuda")
    buf[G:G + n] = float("nan")
    return buf, buf[G:G + n].view(*shape)


def assert_guards(bufs):
    torch.cuda.synchronize()
    for name, (buf, view) in bufs.items():
        host = buf.cpu().numpy()
        assert (host[:G] == 12345.0).all() and (host[-G:] == 12345.0).all(), name
        assert not np.isnan(host[G:-G]).any(), name  # every element of the output was stored


@pytest.mark.parametrize("B", [R + 1, 130])
@pytest.mark.parametrize("H", [64, 320])
def test_nothing_outside_the_outputs_is_written(B, H):
    """The three entry points themselves, every output inside a buffer with G guard elements of a
    sentinel on both sides and NaN inside: the guards stay, every output element is stored."""
    from nmmo_amd import lstm

    T = 3
    L, ptr, stream = lstm.lib(), (lambda t: t.data_ptr()), torch.cuda.current_stream().cuda_stream
    a = cell_inputs(B, H, seed=4)
    out = {k: guarded(B, H) for k in ("h", "c")} | {"act": guarded(B, 4 * H)}
    lstm.check(L.nml_cell(B, H, *[ptr(a[k]) for k in ("ga", "gb", "b_ih", "b_hh", "c_prev")],
                          *[ptr(out[k][1]) for k in ("h", "c", "act")], stream), "nml_cell")
    assert_guards(out)
    for got, want in zip((out[k][1] for k in ("h", "c", "act")), run_cell(**a)):
        assert torch.equal(got, want)

    g = torch.Generator().manual_seed(5)
    mk = lambda *s: torch.randn(*s, generator=g).cuda()  # noqa: E731
    xg, whh, h0, c0 = mk(T, B, 4 * H), mk(4 * H, H) / 8, mk(B, H), mk(B, H)
    fwd = {"y": guarded(T, B, H), "h_T": guarded(B, H), "c_T": guarded(B, H), "gates": guarded(T, B, 4 * H),
           "cs": guarded(T, B, H)}
    lstm.check(L.nml_seq_forward(T, B, H, ptr(xg), ptr(whh.t().contiguous()), ptr(a["b_ih"]), ptr(a["b_hh"]), ptr(h0),
                                 ptr(c0), *[ptr(v[1]) for v in fwd.values()], stream), "nml_seq_forward")
    assert_guards(fwd)
    assert torch.equal(fwd["y"][1][-1], fwd["h_T"][1]) and torch.equal(fwd["cs"][1][-1], fwd["c_T"][1])
    bwd = {"dG": guarded(T, B, 4 * H), "dh0": guarded(B, H), "dc0": guarded(B, H)}
    lstm.check(L.nml_seq_backward(T, B, H, ptr(mk(T, B, H)), ptr(mk(B, H)), ptr(mk(B, H)), ptr(fwd["gates"][1]),
                                  ptr(fwd["cs"][1]), ptr(c0), ptr(whh), *[ptr(v[1]) for v in bwd.values()], stream),
               "nml_seq_backward")
    assert_guards(bwd | fwd)
