"""The fused tile encoder (nmmo_amd/tile.py, csrc/tile_enc.hip) on MI355X against SPEC.md §19.

Forward is checked bit for bit: §19 fixes the order of the 28 float32 additions of an output, so a
numpy float32 restatement (`spec_forward`) reproduces the kernel for any table, and with weights
from {-8..8}/8 every partial sum of either path is exact, so the fused module equals the unfused
torch chain too. Backward is checked exactly where its sums are exact (g_out from {-2..2}/2,
against a float64 `np.add.at`) and, for general inputs, with the project's rule (`within` of
tests/test_gpu_heads.py): the fused path's error against a float64 chain is at most 4 x the error
of the unfused float32 torch chain against the same values.

Row counts 1, 4, 5 and 37: below, equal to and above the forward kernel's 4 rows per workgroup,
and many workgroups with a partial last one.
"""

import ctypes

import numpy as np
import pytest
import torch

from tests.conftest import gpu_available
from tests.test_gpu_heads import within
from tests.test_tile_abi import sample_tiles

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

ROWS = [1, 4, 5, 37]
F32 = np.float32


# ---------------------------------------------------------------- the yardsticks (numpy)
def spec_indices(t):
    """SPEC §19's index rule on float32 [N, 225, 3]: uint8 [N, 225, 3]."""
    t = t.astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        rel = (t[:, :, :2] - t[:, 112:113, :2]).astype(F32) + F32(7.0)
        v = np.concatenate([rel, t[:, :, 2:]], 2)
        idx = np.where(v >= 0, np.trunc(np.minimum(v, F32(255.0))), 0)  # NaN compares false: 0
    return idx.astype(np.uint8)


def spec_forward(idx, table, bias):
    """§19's forward in float32, one addition at a time in the order it fixes: [N, 32, 13, 13]."""
    n = idx.shape[0]
    win = idx.reshape(n, 15, 15, 3)
    z = np.broadcast_to(bias.astype(F32)[None, None, None, :], (n, 13, 13, 32)).copy()
    for ky in range(3):
        for kx in range(3):
            for f in range(3):
                z = (z + table[f][:, ky * 3 + kx, :][win[:, ky:ky + 13, kx:kx + 13, f]]).astype(F32)
    return np.ascontiguousarray(np.maximum(z, F32(0.0)).transpose(0, 3, 1, 2))


def spec_backward(idx, out, g_out):
    """§19's gradients in float64: (g_table [3, 256, 9, 32], g_bias [32])."""
    n = idx.shape[0]
    win = idx.reshape(n, 15, 15, 3)
    dz = np.where(out > 0, g_out, 0).astype(np.float64).transpose(0, 2, 3, 1).reshape(-1, 32)
    g_table = np.zeros((3, 256, 9, 32))
    for ky in range(3):
        for kx in range(3):
            for f in range(3):
                part = np.zeros((256, 32))
                np.add.at(part, win[:, ky:ky + 13, kx:kx + 13, f].reshape(-1), dz)
                g_table[f, :, ky * 3 + kx, :] = part
    return g_table, dz.sum(0)


# ---------------------------------------------------------------- shared inputs
class Case:
    """`n` rows, computed once: integer tiles (the all-zero row, the row centred on coordinate 0,
    the junk row that clips at 0 and 255 with materials 0, 15, 255), general and exact weights."""

    def __init__(self, n):
        from nmmo_amd import tile

        rng = np.random.default_rng(100 + n)
        self.n = n
        tiles = sample_tiles(max(n, 3), rng)
        self.tiles = tiles[[2, 0, 1][:n]] if n < 3 else tiles  # one row: the junk row
        self.idx = spec_indices(self.tiles)
        self.table = rng.standard_normal((3, 256, 9, 32)).astype(F32)
        self.bias = rng.standard_normal(32).astype(F32)
        self.want = spec_forward(self.idx, self.table, self.bias)
        self.g_exact = (rng.integers(-2, 3, self.want.shape) / 2).astype(F32)
        self.x = torch.from_numpy(self.tiles).cuda()
        self.table_t, self.bias_t = torch.from_numpy(self.table).cuda(), torch.from_numpy(self.bias).cuda()
        self.tile = tile


_cases = {}


def case(n):
    if n not in _cases:
        _cases[n] = Case(n)
    return _cases[n]


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def run_forward(c, x, stride, kind, out, idx_out):
    from nmmo_amd import heads

    heads.check(heads.lib().nmh_tile_forward(c.n, ptr(x), stride, kind, ptr(c.table_t), ptr(c.bias_t), ptr(out),
                                             None if idx_out is None else ptr(idx_out), None), "nmh_tile_forward")
    torch.cuda.synchronize()


def run_backward(c, idx, out, g_out, n_chunks):
    """(g_table_parts, g_bias_parts), both NaN before the call"""
    from nmmo_amd import heads

    parts = torch.full((n_chunks, 3, 256, 9, 32), float("nan"), device="cuda")
    bparts = torch.full((n_chunks, 32), float("nan"), device="cuda")
    heads.check(heads.lib().nmh_tile_backward(c.n, ptr(idx), ptr(out), ptr(g_out), n_chunks, ptr(parts), ptr(bparts),
                                              None), "nmh_tile_backward")
    torch.cuda.synchronize()
    return parts, bparts


def saved(c):
    """(idx uint8, out) of the general-table forward on the GPU, as backward's inputs"""
    if not hasattr(c, "_saved"):
        out = torch.empty((c.n, 32, 13, 13), device="cuda")
        idx = torch.empty((c.n, 225, 3), dtype=torch.uint8, device="cuda")
        run_forward(c, c.x, 675, c.tile.TILE_F32, out, idx)
        c._saved = (idx, out)
    return c._saved


# ---------------------------------------------------------------- 1. forward, general tables
def test_the_cases_hold_the_edge_rows():
    c = case(37)
    assert not c.tiles[0].any() and (c.idx[0, :, :2] == 7).all() and (c.idx[0, :, 2] == 0).all()
    assert c.tiles[1, 112, 0] == 0 and c.tiles[1, 0, 0] == -7 and c.idx[1, 0, 0] == 0 and c.idx[1, 224, 1] == 14
    assert (c.idx[2] == 0).any() and (c.idx[2] == 255).any() and list(c.idx[2, :4, 2]) == [0, 15, 255, 255]
    assert case(1).idx.min() == 0 and case(1).idx.max() == 255


@pytest.mark.parametrize("n", ROWS)
def test_forward_equals_the_float32_restatement_bit_for_bit(n):
    c = case(n)
    got = c.tile.tile_conv1(c.x, c.table_t, c.bias_t)
    assert got.shape == (n, 32, 13, 13) and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy().view(np.uint32), c.want.view(np.uint32))
    idx, out = saved(c)
    assert np.array_equal(idx.cpu().numpy(), c.idx)
    assert torch.equal(out, got)
    # the int16 rows that hold the same integers give the same bits
    got16 = c.tile.tile_conv1(c.x.to(torch.int16), c.table_t, c.bias_t)
    assert torch.equal(got16.view(torch.int32), got.view(torch.int32))
    idx16 = torch.empty_like(idx)
    run_forward(c, c.x.to(torch.int16), 675, c.tile.TILE_I16, torch.empty_like(out), idx16)
    assert torch.equal(idx16, idx)


def test_forward_float_coordinates_follow_the_index_rule():
    """fractions truncate toward zero, NaN gives 0, infinities and huge values clamp"""
    c = case(5)
    t = c.tiles.copy()
    t[3, :8, 0] = [3.7, -0.5, np.nan, np.inf, -np.inf, 1e30, -1e30, 254.99]
    t[3, 8:12, 2] = [np.nan, 255.5, 15.99, -0.99]
    t[4, 112, 0] = np.nan  # a NaN centre: the whole feature column is NaN, index 0
    t[4, 112, 1] = 0.25
    idx = spec_indices(t)
    assert (idx[4, :, 0] == 0).all() and list(idx[3, 8:12, 2]) == [0, 255, 15, 0]
    want = spec_forward(idx, c.table, c.bias)
    out = torch.empty((5, 32, 13, 13), device="cuda")
    got_idx = torch.empty((5, 225, 3), dtype=torch.uint8, device="cuda")
    run_forward(c, torch.from_numpy(t).cuda(), 675, c.tile.TILE_F32, out, got_idx)
    assert np.array_equal(got_idx.cpu().numpy(), idx)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------- 2. forward, exact inputs
def exact_encoders(seed=3):
    from nmmo_amd.tile import TileEncoder

    g = torch.Generator().manual_seed(seed)
    fused, unfused = TileEncoder(32, fused=True), TileEncoder(32, fused=False)
    with torch.no_grad():
        for p in (fused.embedding.weight, fused.tile_conv_1.weight, fused.tile_conv_1.bias):
            p.copy_(torch.randint(-8, 9, p.shape, generator=g) / 8.0)
    unfused.load_state_dict(fused.state_dict())
    return fused.cuda(), unfused.cuda()


@pytest.mark.parametrize("n", ROWS)
def test_fused_module_equals_the_unfused_chain_bit_for_bit_on_exact_weights(n):
    c = case(n)
    fused, unfused = exact_encoders()
    with torch.no_grad():
        got, want = fused.conv1(c.x), unfused.conv1(c.x)
    assert got.shape == want.shape == (n, 32, 13, 13) and float(want.max()) > 0
    assert torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32))


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
    # through the module function: the view's memory is what the kernel reads
    got = c.tile.tile_conv1(view, c.table_t, c.bias_t)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), c.want.view(np.uint32))
    # through the C interface, the outputs inside canary margins
    lo, hi = 61, 67
    big = torch.full((lo + n * 5408 + hi,), -123.25, device="cuda")
    bigi = torch.full((37 + n * 675 + 41,), 0xA5, dtype=torch.uint8, device="cuda")
    out, idx = big[lo:lo + n * 5408], bigi[37:37 + n * 675]
    run_forward(c, view, E, c.tile.TILE_F32 if kind == "f32" else c.tile.TILE_I16, out, idx)
    assert torch.equal(buf.view(torch.int16), keep.view(torch.int16))
    assert np.array_equal(out.cpu().numpy().view(np.uint32).reshape(c.want.shape), c.want.view(np.uint32))
    assert np.array_equal(idx.cpu().numpy().reshape(n, 225, 3), c.idx)
    assert (big[:lo] == -123.25).all() and (big[lo + n * 5408:] == -123.25).all()
    assert (bigi[:37] == 0xA5).all() and (bigi[37 + n * 675:] == 0xA5).all()


def test_no_grad_forward_saves_nothing_and_grad_forward_survives_an_obs_rewrite():
    c = case(5)
    table = c.table_t.clone().requires_grad_(True)
    with torch.no_grad():
        assert c.tile.tile_conv1(c.x, table, c.bias_t).grad_fn is None
    x = c.x.clone()
    out = c.tile.tile_conv1(x, table, c.bias_t)
    x.fill_(9.0)  # the next step rewrites the obs buffer: backward reads its own copy of the indices
    g = torch.from_numpy(c.g_exact).cuda()
    out.backward(g)
    want, _ = spec_backward(c.idx, c.want, c.g_exact)
    assert np.array_equal(table.grad.double().cpu().numpy(), want)


# ---------------------------------------------------------------- 4. backward, exact inputs
@pytest.mark.parametrize("n", ROWS)
def test_backward_sums_equal_float64_exactly_for_every_chunking(n):
    c = case(n)
    idx, out = saved(c)
    g = torch.from_numpy(c.g_exact).cuda()
    want_t, want_b = spec_backward(c.idx, c.want, c.g_exact)
    assert np.abs(want_t).max() > 1
    for n_chunks in (1, 2, 3, n + 2):
        parts, bparts = run_backward(c, idx, out, g, n_chunks)
        assert torch.isfinite(parts).all() and torch.isfinite(bparts).all(), n_chunks  # every entry written
        assert np.array_equal(parts.sum(0).double().cpu().numpy(), want_t), n_chunks
        assert np.array_equal(bparts.sum(0).double().cpu().numpy(), want_b), n_chunks
        rows = -(-n // n_chunks)  # chunk c owns rows [c rows, min(n, (c + 1) rows))
        for ch in range(n_chunks):
            lo, hi = min(n, ch * rows), min(n, (ch + 1) * rows)
            if lo == hi:
                assert not parts[ch].any() and not bparts[ch].any(), (n_chunks, ch)
            else:
                _, b = spec_backward(c.idx[lo:hi], c.want[lo:hi], c.g_exact[lo:hi])
                assert np.array_equal(bparts[ch].double().cpu().numpy(), b), (n_chunks, ch)
        if n_chunks == n + 2:
            assert not parts[n:].any()


# ---------------------------------------------------------------- 5. backward, general inputs
@pytest.mark.parametrize("n", [5, 37])
def test_parameter_gradients_stay_within_the_unfused_chains_error(n):
    from nmmo_amd.tile import TileEncoder

    c = case(n)
    torch.manual_seed(7)
    master = TileEncoder(24)
    w = torch.randn((n, 24), generator=torch.Generator().manual_seed(8))

    def grads(fused, dtype, device):
        enc = TileEncoder(24, fused=fused)
        enc.load_state_dict(master.state_dict())
        enc = enc.to(device=device, dtype=dtype)
        x = torch.from_numpy(c.tiles).to(device=device, dtype=dtype)
        (enc(x) * w.to(device=device, dtype=dtype)).sum().backward()
        return {k: p.grad.double().cpu().numpy() for k, p in enc.named_parameters()}

    want = grads(False, torch.float64, "cpu")
    g_unfused, g_fused = grads(False, torch.float32, "cuda"), grads(True, torch.float32, "cuda")
    assert set(g_fused) == set(want) and len(want) == 7
    for name in ("embedding.weight", "tile_conv_1.weight", "tile_conv_1.bias"):
        assert np.abs(want[name]).max() > 0
        within(f"n={n} grad {name}", g_fused[name], want[name], g_unfused[name])


# ---------------------------------------------------------------- 6. determinism
def test_two_backward_calls_give_identical_bits():
    c = case(37)
    idx, out = saved(c)
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(9)).cuda()
    for n_chunks in (1, 3):
        a, ab = run_backward(c, idx, out, g, n_chunks)
        b, bb = run_backward(c, idx, out, g, n_chunks)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert torch.equal(ab.view(torch.int32), bb.view(torch.int32))
    table = c.table_t.clone().requires_grad_(True)
    bits = []
    for _ in range(2):
        table.grad = None
        c.tile.tile_conv1(c.x, table, c.bias_t).backward(g)
        bits.append(table.grad.view(torch.int32).clone())
    assert torch.equal(bits[0], bits[1])
