"""The tile encoder with its second convolution fused in (nmmo_amd/tile.py `tile_conv12`,
csrc/tile_enc.hip nmh_tile2_forward / nmh_tile2_backward) on MI355X against SPEC.md §22.

Forward is checked bit for bit: §22 fixes the order of the 288 multiply-adds of an output (c, ky, kx
ascending) on top of §19's 28 additions, so the numpy float32 restatement of
tests/test_tile_conv2_abi.py reproduces the kernel for any table and weights. With the exact weights
of `exact_state` (embedding from {-1, 0, 1}; tile_conv_1.weight, both biases, tile_conv_2.weight from
{-2..2}/2) |a1| <= 865 in multiples of 1/2 and |z2| < 2.5e5 in multiples of 1/4, so every partial sum
is exact in any order and the three modules (`fused_conv2`, `fused`, unfused torch) agree bit for
bit. That exactness was confirmed on the CPU first: the float32 restatement, the float32 torch chain
and the float64 torch chain are equal value for value
(test_tile_conv2_abi.test_restatement_equals_the_float64_chain_bit_for_bit_on_exact_weights).
Backward is checked exactly where its sums are exact (those weights, g_out2 from {-2..2}/2, N <= 37:
|dz1| <= 72 and |g_W2| <= 865 x 121 x 37 = 3.9e6 in multiples of 1/4, below 2^24 of that unit) against
the float64 restatement, and for general inputs with the project's rule (`within` of
tests/test_gpu_heads.py): the fused path's error against a float64 chain is at most 4 x the error of
the unfused float32 torch chain against the same values.

Row counts 1, 3, 4, 5 and 37: one, then below, equal to and above the forward kernel's 4 rows per
workgroup (which is also `n_w2_parts_for`'s 4 rows per part), and many workgroups with a partial
last one.
"""

import ctypes

import numpy as np
import pytest
import torch

from tests.conftest import gpu_available
from tests.test_gpu_heads import within
from tests.test_gpu_learner_fullsize import grows
from tests.test_tile_abi import sample_tiles
from tests.test_tile_conv2_abi import exact_state, spec2_backward, spec2_forward, spec_a1, spec_indices

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

ROWS = [1, 3, 4, 5, 37]
F32 = np.float32
U8 = torch.uint8


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------- shared inputs
class Case:
    """`n` rows, computed once: integer tiles (the all-zero row, the row centred on coordinate 0,
    the junk row that clips at 0 and 255), a general table and weights with the restatement's
    outputs, and the exact weights with theirs."""

    def __init__(self, n):
        from nmmo_amd import tile

        assert tile.FWD2_ROWS == 4 and ROWS[1:4] == [tile.FWD2_ROWS - 1, tile.FWD2_ROWS, tile.FWD2_ROWS + 1]
        rng = np.random.default_rng(200 + n)
        self.n, self.tile = n, tile
        tiles = sample_tiles(max(n, 3), rng)
        self.tiles = tiles[[2, 0, 1][:n]] if n < 3 else tiles  # one row: the junk row
        self.idx = spec_indices(self.tiles)
        self.x = dev(self.tiles)
        # general
        self.table = rng.standard_normal((3, 256, 9, 32)).astype(F32)
        self.bias1 = rng.standard_normal(32).astype(F32)
        self.w2 = (rng.standard_normal((8, 32, 3, 3)) / 8).astype(F32)
        self.bias2 = rng.standard_normal(8).astype(F32)
        self.a1 = spec_a1(self.idx, self.table, self.bias1)
        self.want = spec2_forward(self.a1, self.w2, self.bias2)
        self.general = tuple(dev(a) for a in (self.table, self.bias1, self.w2, self.bias2))
        # exact
        sd = exact_state()
        self.sd = sd
        self.e_table = tile.tile_table(sd["embedding.weight"], sd["tile_conv_1.weight"]).numpy()
        self.e_bias1, self.e_w2, self.e_bias2 = (sd[k].numpy() for k in ("tile_conv_1.bias", "tile_conv_2.weight",
                                                                         "tile_conv_2.bias"))
        self.e_a1 = spec_a1(self.idx, self.e_table, self.e_bias1)
        self.e_out2 = spec2_forward(self.e_a1, self.e_w2, self.e_bias2)
        self.e_g = (rng.integers(-2, 3, self.e_out2.shape) / 2).astype(F32)
        self.exact = tuple(dev(a) for a in (self.e_table, self.e_bias1, self.e_w2, self.e_bias2))
        self._parts = {}

    def want_backward(self, lo, hi):
        """§22's float64 gradients of the exact case over rows [lo, hi)"""
        if (lo, hi) not in self._parts:
            self._parts[lo, hi] = spec2_backward(self.idx[lo:hi], self.e_a1[lo:hi], self.e_out2[lo:hi], self.e_g[lo:hi],
                                                 self.e_w2)[:4]
        return self._parts[lo, hi]


_cases = {}


def case(n):
    if n not in _cases:
        _cases[n] = Case(n)
    return _cases[n]


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def run_forward(n, x, stride, kind, weights, out2, idx_out):
    from nmmo_amd import heads

    table, bias1, w2, bias2 = weights
    heads.check(heads.lib().nmh_tile2_forward(n, ptr(x), stride, kind, ptr(table), ptr(bias1), ptr(w2), ptr(bias2),
                                              ptr(out2), ptr(idx_out), None), "nmh_tile2_forward")
    torch.cuda.synchronize()


def run_backward(c, g_out2, n_chunks, n_parts, weights=None, out2=None):
    """(g_table_parts, g_bias1_parts, g_w2_parts, g_bias2_parts) of the exact case, all NaN before the call"""
    from nmmo_amd import heads

    table, bias1, w2, _ = weights or c.exact
    out2 = dev(c.e_out2) if out2 is None else out2

    def nan(*shape):
        return torch.full(shape, float("nan"), device="cuda")

    scratch = nan(c.n, 32, 13, 13)
    outs = nan(n_chunks, 3, 256, 9, 32), nan(n_chunks, 32), nan(n_parts, 8, 32, 3, 3), nan(n_parts, 8)
    heads.check(heads.lib().nmh_tile2_backward(c.n, ptr(dev(c.idx)), ptr(out2), ptr(g_out2), ptr(table), ptr(bias1), ptr(w2),
                                               n_chunks, n_parts, ptr(scratch), *[ptr(t) for t in outs], None),
                "nmh_tile2_backward")
    torch.cuda.synchronize()
    return outs


def same_bits(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), np.ascontiguousarray(want, dtype=F32).view(np.uint32)), what


# ---------------------------------------------------------------- 1. forward, general weights
def test_the_cases_hold_the_edge_rows_and_both_signs():
    c = case(37)
    assert not c.tiles[0].any() and (c.idx[0, :, :2] == 7).all() and (c.idx[0, :, 2] == 0).all()
    assert c.tiles[1, 112, 0] == 0 and c.idx[1, 0, 0] == 0 and c.idx[1, 224, 1] == 14
    assert (c.idx[2] == 0).any() and (c.idx[2] == 255).any()
    for out in (c.a1, c.want, c.e_a1, c.e_out2):
        assert (out > 0).any() and (out == 0).any()  # the ReLUs gate some and pass some
    assert np.abs(c.e_a1).max() <= 865 and np.abs(c.e_out2).max() < 2.5e5


@pytest.mark.parametrize("n", ROWS)
def test_forward_equals_the_float32_restatement_bit_for_bit(n):
    c = case(n)
    got = c.tile.tile_conv12(c.x, *c.general)
    assert got.shape == (n, 8, 11, 11) and got.is_contiguous() and got.grad_fn is None
    same_bits(got, c.want, "tile_conv12")
    out2, idx = torch.empty_like(got), torch.empty((n, 225, 3), dtype=U8, device="cuda")
    run_forward(n, c.x, 675, c.tile.TILE_F32, c.general, out2, idx)
    same_bits(out2, c.want, "C call")
    assert np.array_equal(idx.cpu().numpy(), c.idx)  # §19's indices
    no_idx = torch.empty_like(got)
    run_forward(n, c.x, 675, c.tile.TILE_F32, c.general, no_idx, None)
    assert torch.equal(bits(no_idx), bits(out2))
    # the int16 rows that hold the same integers give the same bits
    x16 = c.x.to(torch.int16)
    out16, idx16 = torch.empty_like(got), torch.empty_like(idx)
    run_forward(n, x16, 675, c.tile.TILE_I16, c.general, out16, idx16)
    assert torch.equal(bits(out16), bits(out2)) and torch.equal(idx16, idx)
    assert torch.equal(bits(c.tile.tile_conv12(x16, *c.general)), bits(out2))
    # a1 is §19's `out`, bit for bit
    same_bits(c.tile.tile_conv1(c.x, c.general[0], c.general[1]), c.a1, "a1")


# ---------------------------------------------------------------- 2. the modules, exact weights
def exact_encoders():
    from nmmo_amd.tile import TileEncoder

    encs = [TileEncoder(32, fused=True, fused_conv2=True), TileEncoder(32, fused=True), TileEncoder(32)]
    for e in encs:
        e.load_state_dict(exact_state())
    return [e.cuda() for e in encs]


@pytest.mark.parametrize("n", ROWS)
def test_the_three_modules_agree_bit_for_bit_on_exact_weights(n):
    c = case(n)
    both, first, none = exact_encoders()
    with torch.no_grad():
        got = c.tile.tile_conv12(c.x, *c.exact)
        same_bits(got, c.e_out2, "tile_conv12, exact weights")
        for enc in (first, none):
            want = torch.relu(enc.tile_conv_2(enc.conv1(c.x)))
            assert torch.equal(bits(got), bits(want)), "fused" if enc is first else "unfused"
        h = both(c.x)
        assert h.shape == (n, 32) and float(h.max()) > 0
        assert torch.equal(bits(h), bits(first(c.x))) and torch.equal(bits(h), bits(none(c.x)))


# ---------------------------------------------------------------- 3. in-place read
@pytest.mark.parametrize("kind", ["f32", "i16"])
def test_rows_are_read_in_place_and_nothing_else_is_written(kind):
    c = case(5)
    E, off, n = 701, 13, 5  # odd row width: the rows are not 16-byte aligned
    dtype = torch.float32 if kind == "f32" else torch.int16
    g = torch.Generator().manual_seed(4)
    buf = torch.randint(-300, 300, (n, E), generator=g).to(dtype).cuda()
    buf[:, off:off + 675] = c.x.reshape(n, 675).to(dtype)
    keep = buf.clone()
    view = buf[:, off:off + 675]
    assert view.stride(0) == E and view.data_ptr() % 16 != 0
    arg, stride, _ = c.tile._tile_arg(view, None)
    assert arg.data_ptr() == view.data_ptr() and stride == E  # the view's own memory is what the kernel reads
    same_bits(c.tile.tile_conv12(view, *c.general), c.want, "view")
    # through the C interface, the outputs inside canary margins
    lo, hi = 61, 67
    big = torch.full((lo + n * 968 + hi,), -123.25, device="cuda")
    bigi = torch.full((37 + n * 675 + 41,), 0xA5, dtype=U8, device="cuda")
    out2, idx = big[lo:lo + n * 968], bigi[37:37 + n * 675]
    run_forward(n, view, E, c.tile.TILE_F32 if kind == "f32" else c.tile.TILE_I16, c.general, out2, idx)
    assert torch.equal(buf.view(torch.int16), keep.view(torch.int16))
    same_bits(out2.reshape(n, 8, 11, 11), c.want, "C call on the view")
    assert np.array_equal(idx.cpu().numpy().reshape(n, 225, 3), c.idx)
    assert (big[:lo] == -123.25).all() and (big[lo + n * 968:] == -123.25).all()
    assert (bigi[:37] == 0xA5).all() and (bigi[37 + n * 675:] == 0xA5).all()


# ---------------------------------------------------------------- 4. memory
def test_forward_allocates_its_output_and_keeps_only_indices_and_output():
    """The [N, 32, 13, 13] activation would be 800,384 B at 37 rows; out2 is 143,264 B and idx 24,975 B."""
    c = case(37)
    n = c.n
    table, bias1, w2, bias2 = (t.clone() for t in c.exact)
    with torch.no_grad(), grows(True, "tile_conv12 without grad", ((n, 8, 11, 11), torch.float32)):
        out = c.tile.tile_conv12(c.x, table, bias1, w2, bias2)
    assert out.grad_fn is None
    del out
    for t in (table, bias1, w2, bias2):
        t.requires_grad_(True)
    x = c.x.clone()
    with grows(True, "tile_conv12 with grad", ((n, 8, 11, 11), torch.float32), ((n, 225, 3), U8)):
        out = c.tile.tile_conv12(x, table, bias1, w2, bias2)
    kept = out.grad_fn.saved_tensors
    inputs = {t.data_ptr() for t in (table, bias1, w2, bias2)}
    own = [t for t in kept if t.data_ptr() not in inputs]
    assert sorted((tuple(t.shape), t.dtype) for t in own) == sorted([((n, 225, 3), U8), ((n, 8, 11, 11), torch.float32)])
    assert all(t.data_ptr() != x.data_ptr() for t in kept)
    x.fill_(9.0)  # the next step rewrites the obs buffer: backward reads its own copy of the indices
    out.backward(dev(c.e_g))
    want = c.want_backward(0, n)
    for name, t, w in zip(("table", "bias1", "w2", "bias2"), (table, bias1, w2, bias2), want):
        assert np.array_equal(t.grad.double().cpu().numpy(), w), name


# ---------------------------------------------------------------- 5. backward, exact inputs
@pytest.mark.parametrize("n", ROWS)
def test_backward_sums_equal_float64_exactly_for_every_split(n):
    """The table chunks belong to the second launch and the W2 parts to the first, so the two counts
    are varied together: (1, 1), (2, 2), (64, the cap)."""
    c = case(n)
    g = dev(c.e_g)
    want = c.want_backward(0, n)
    assert all(np.abs(w).max() > 1 for w in want)
    for n_chunks, n_parts in ((1, 1), (2, 2), (64, c.tile.MAX_W2_PARTS)):
        got = run_backward(c, g, n_chunks, n_parts)
        for name, t, w in zip(("g_table", "g_bias1", "g_w2", "g_bias2"), got, want):
            assert torch.isfinite(t).all(), (name, n_chunks, n_parts)  # every entry written
            assert np.array_equal(t.sum(0).double().cpu().numpy(), w), (name, n_chunks, n_parts)
        for count, (t_big, t_small), pick in ((n_chunks, got[:2], (0, 1)), (n_parts, got[2:], (2, 3))):
            rows = -(-n // count)  # part p owns rows [p rows, min(n, (p + 1) rows))
            big, small = t_big.double().cpu().numpy(), t_small.double().cpu().numpy()
            for p in range(count):
                lo, hi = min(n, p * rows), min(n, (p + 1) * rows)
                if lo == hi:
                    assert not big[p].any() and not small[p].any(), (n_chunks, n_parts, p)
                else:
                    w = c.want_backward(lo, hi)
                    assert np.array_equal(big[p], w[pick[0]]) and np.array_equal(small[p], w[pick[1]]), (count, p)


# ---------------------------------------------------------------- 6. backward, general inputs
@pytest.mark.parametrize("n", [5, 37])
def test_parameter_gradients_stay_within_the_unfused_chains_error(n):
    from nmmo_amd.tile import TileEncoder

    c = case(n)
    torch.manual_seed(7)
    master = TileEncoder(24)
    w = torch.randn((n, 24), generator=torch.Generator().manual_seed(8))

    def grads(fused, dtype, device):
        enc = TileEncoder(24, fused=fused, fused_conv2=fused)
        enc.load_state_dict(master.state_dict())
        enc = enc.to(device=device, dtype=dtype)
        x = torch.from_numpy(c.tiles).to(device=device, dtype=dtype)
        out = enc(x)
        (out * w.to(device=device, dtype=dtype)).sum().backward()
        return out.detach().double().cpu().numpy(), {k: p.grad.double().cpu().numpy() for k, p in enc.named_parameters()}

    out_want, want = grads(False, torch.float64, "cpu")
    (out_unfused, g_unfused), (out_fused, g_fused) = grads(False, torch.float32, "cuda"), grads(True, torch.float32, "cuda")
    within(f"n={n} output", out_fused, out_want, out_unfused)
    assert set(g_fused) == set(want) and len(want) == 7
    for name in want:
        assert np.abs(want[name]).max() > 0
        within(f"n={n} grad {name}", g_fused[name], want[name], g_unfused[name])


# ---------------------------------------------------------------- 7. determinism
def test_two_backward_calls_give_identical_bits():
    c = case(37)
    out2 = dev(c.want)
    g = torch.randn(out2.shape, generator=torch.Generator().manual_seed(9)).cuda()
    for n_chunks, n_parts in ((1, 1), (3, 10)):
        a = run_backward(c, g, n_chunks, n_parts, c.general, out2)
        b = run_backward(c, g, n_chunks, n_parts, c.general, out2)
        for s, t in zip(a, b):
            assert torch.isfinite(s).all() and torch.equal(bits(s), bits(t))
    params = [t.clone().requires_grad_(True) for t in c.general]
    seen = []
    for _ in range(2):
        for p in params:
            p.grad = None
        c.tile.tile_conv12(c.x, *params).backward(g)
        seen.append([bits(p.grad).clone() for p in params])
    assert all(torch.equal(s, t) for s, t in zip(*seen))
