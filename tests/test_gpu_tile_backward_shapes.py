"""nmh_tile_backward (nmmo_amd/csrc/tile_enc.hip, SPEC.md §19) at a minibatch's row counts.

`tile_conv1` sums the table gradient over n_chunks_for(N) = min(64, ceil(N / 16)) chunks of rows.
tests/test_gpu_tile.py stops at 37 rows and 3 chunks; here the cap itself (N = 1,024: 64 chunks of
16 rows), the first N past it (1,025: 17 rows per chunk, chunk 60 holds 5 rows, chunks 61 to 63 are
empty) and 1,088 (64 full chunks of 17 rows). tests/test_tile_chunks.py pins that geometry on the
CPU.

a. Exact sums. g_out from {-2..2}/2 makes every partial sum a multiple of 0.5 bounded by
   1,088 x 169 x 1 < 2^23, so float32 sums are exact in any order, and the kernel's parts, their sum
   and `tile_conv1`'s gradients must equal a float64 scatter with `np.array_equal`. Rows 3..258
   carry materials that cover 0..255, so every owner of the backward kernel (wave v & 7, half
   (v >> 3) & 1) adds entries. The float64 scatter is `index_add_` (np.add.at is too slow here) and
   is itself pinned to test_gpu_tile.spec_backward at 37 rows.
b. General gradients at N = 1,040 (a minibatch), the three parameter gradients of `TileEncoder`
   under `within`: the float64 CPU chain is `want`, the unfused float32 GPU chain gives E_ref. Two
   inputs: `sample_tiles` rows, and concentrated rows (every agent at the same map position, one
   material in all 225 tiles), where the material's entry of every (feature 2, tap) slice takes all
   169 x 17 float32 additions of a chunk in one serial chain.
c. Two calls give the same bits at N = 1,025, directly and through autograd.

Measured on an MI355X at N = 1,040, fused err / E_ref = ratio (the bound is 4):
                         sampled rows                        concentrated rows
  embedding.weight       5.97e-07 / 3.18e-04 = 0.002         2.02e-06 / 6.90e-06 = 0.29
  tile_conv_1.weight     6.56e-06 / 1.01e-02 = 0.001         1.49e-05 / 3.96e-05 = 0.38
  tile_conv_1.bias       1.73e-06 / 3.49e-03 = 0.0005        2.04e-06 / 9.39e-07 = 2.18
The serial float32 chain of 169 x 17 additions does not show: the fused error is about the same on
both inputs (gradients of magnitude 1 to 18), and the rule holds with room, so the chunking and
`_TileConv1.backward` stay as they are. What moves is E_ref: on sampled rows the unfused float32
chain is three orders of magnitude less accurate than on concentrated rows. The first run of the
unfused chain at this row count on a machine spends about 8 s choosing its convolution kernels;
after that the test takes under a second.
"""

from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.conftest import gpu_available
from tests.test_gpu_heads import within
from tests.test_gpu_tile import run_backward, run_forward, spec_backward, spec_forward, spec_indices
from tests.test_tile_abi import sample_tiles
from tests.test_tile_chunks import CAP_CASES, chunk_rows, empty_chunks

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

F32 = np.float32
N_MAX = max(CAP_CASES)


# ---------------------------------------------------------------- the float64 scatter
def scatter_backward(idx, out, g_out):
    """§19's gradients in float64, as test_gpu_tile.spec_backward, with index_add_ for np.add.at:
    (g_table [3, 256, 9, 32], g_bias [32]) as numpy arrays."""
    n = idx.shape[0]
    win = torch.from_numpy(idx.reshape(n, 15, 15, 3).astype(np.int64))
    dz = torch.from_numpy(np.where(out > 0, g_out, 0).astype(np.float64).transpose(0, 2, 3, 1).reshape(-1, 32))
    g_table = torch.zeros((3, 256, 9, 32), dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            for f in range(3):
                part = torch.zeros((256, 32), dtype=torch.float64)
                part.index_add_(0, win[:, ky:ky + 13, kx:kx + 13, f].reshape(-1), dz)
                g_table[f, :, ky * 3 + kx, :] = part
    return g_table.numpy(), dz.sum(0).numpy()


_shared = {}


def rows():
    """N_MAX rows, computed once; the cases use the first N. `sample_tiles` rows, with the material
    of rows 3..258 running through all 256 values."""
    if not _shared:
        from nmmo_amd import tile

        rng = np.random.default_rng(1088)
        tiles = sample_tiles(N_MAX, rng)
        tiles[3:259, :, 2] = (np.arange(256)[:, None] + 37 * np.arange(225)[None, :]) % 256
        idx = spec_indices(tiles)
        table = rng.standard_normal((3, 256, 9, 32)).astype(F32)
        bias = rng.standard_normal(32).astype(F32)
        want = spec_forward(idx, table, bias)
        g_exact = (rng.integers(-2, 3, want.shape) / 2).astype(F32)
        c = SimpleNamespace(n=N_MAX, tile=tile, tiles=tiles, idx=idx, table=table, bias=bias, want=want, g_exact=g_exact,
                            x=torch.from_numpy(tiles).cuda(), table_t=torch.from_numpy(table).cuda(),
                            bias_t=torch.from_numpy(bias).cuda(), g_t=torch.from_numpy(g_exact).cuda())
        c.out_t = torch.empty((N_MAX, 32, 13, 13), device="cuda")
        c.idx_t = torch.empty((N_MAX, 225, 3), dtype=torch.uint8, device="cuda")
        run_forward(c, c.x, 675, tile.TILE_F32, c.out_t, c.idx_t)
        _shared["c"] = c
    return _shared["c"]


def first(c, n):
    """the first n rows as a case of their own (views)"""
    return SimpleNamespace(n=n, tile=c.tile, idx=c.idx[:n], want=c.want[:n], g_exact=c.g_exact[:n], x=c.x[:n],
                           table_t=c.table_t, bias_t=c.bias_t, g_t=c.g_t[:n], out_t=c.out_t[:n], idx_t=c.idx_t[:n])


def test_the_rows_reach_every_owner_and_the_forward_is_the_restatements():
    c = rows()
    assert set(np.unique(c.idx[3:259, :, 2])) == set(range(256))
    owners = {(v & 7, (v >> 3) & 1) for v in range(256)}
    assert len(owners) == 16
    assert np.array_equal(c.idx_t.cpu().numpy(), c.idx)
    assert np.array_equal(c.out_t.cpu().numpy().view(np.uint32), c.want.view(np.uint32))
    assert (c.want > 0).mean() > 0.2


def test_the_scatter_is_spec_backward():
    c = first(rows(), 37)
    (t, b), (wt, wb) = scatter_backward(c.idx, c.want, c.g_exact), spec_backward(c.idx, c.want, c.g_exact)
    assert np.array_equal(t, wt) and np.array_equal(b, wb) and np.abs(wt).max() > 1


# ---------------------------------------------------------------- a. exact sums at the cap
@pytest.mark.parametrize("n", sorted(CAP_CASES))
def test_backward_sums_are_exact_at_the_cap(n):
    c = first(rows(), n)
    chunks, R, last_rows, empty = CAP_CASES[n]
    assert c.tile.n_chunks_for(n) == chunks and empty_chunks(n, chunks) == empty
    want_t, want_b = scatter_backward(c.idx, c.want, c.g_exact)
    assert np.abs(want_t).max() > 8 and np.abs(want_t).max() * 2 < 2 ** 23
    parts, bparts = run_backward(c, c.idx_t, c.out_t, c.g_t, chunks)
    assert torch.isfinite(parts).all() and torch.isfinite(bparts).all()  # every entry written over the NaN
    assert np.array_equal(parts.sum(0).double().cpu().numpy(), want_t)
    assert np.array_equal(bparts.sum(0).double().cpu().numpy(), want_b)
    k_last = chunks - empty - 1
    parts_h, bparts_h = parts.double().cpu().numpy(), bparts.double().cpu().numpy()
    for k in range(chunks):
        lo, hi = chunk_rows(n, chunks, k)
        if lo >= hi:
            assert k > k_last and not parts_h[k].any() and not bparts_h[k].any(), k
            continue
        assert hi - lo == (last_rows if k == k_last else R), k
        if k in (0, chunks // 2 - 1, k_last):  # the first, a middle and the last chunk that holds rows
            t, b = scatter_backward(c.idx[lo:hi], c.want[lo:hi], c.g_exact[lo:hi])
            assert np.array_equal(parts_h[k], t), k
        else:
            b = np.where(c.want[lo:hi] > 0, c.g_exact[lo:hi], 0).astype(np.float64).sum((0, 2, 3))
        assert np.array_equal(bparts_h[k], b), k
    assert sum(1 for k in range(chunks) if not parts_h[k].any()) == empty
    # the same values through autograd
    table, bias = c.table_t.clone().requires_grad_(True), c.bias_t.clone().requires_grad_(True)
    out = c.tile.tile_conv1(c.x, table, bias)
    assert torch.equal(out.view(torch.int32), c.out_t.view(torch.int32))
    out.backward(c.g_t)
    assert np.array_equal(table.grad.double().cpu().numpy(), want_t)
    assert np.array_equal(bias.grad.double().cpu().numpy(), want_b)


# ---------------------------------------------------------------- b. general gradients at 1,040 rows
N_BATCH = 1040


def concentrated_tiles(n):
    """every agent at map position (40, 90), material 5 in all 225 tiles of every row"""
    yy, xx = np.meshgrid(np.arange(15), np.arange(15), indexing="ij")
    t = np.zeros((n, 225, 3), dtype=F32)
    t[:, :, 0], t[:, :, 1], t[:, :, 2] = (40 + yy).ravel(), (90 + xx).ravel(), 5
    return t


@pytest.mark.parametrize("kind", ["sampled", "concentrated"])
def test_parameter_gradients_stay_within_the_unfused_chains_error_at_a_minibatch(kind):
    from nmmo_amd.tile import TileEncoder, n_chunks_for

    n = N_BATCH
    assert n_chunks_for(n) == 64 and -(-n // 64) == 17
    tiles = sample_tiles(n, np.random.default_rng(1040)) if kind == "sampled" else concentrated_tiles(n)
    if kind == "concentrated":
        idx = spec_indices(tiles)
        assert (idx == idx[0]).all() and (idx[0, :, 2] == 5).all()
    torch.manual_seed(7)
    master = TileEncoder(24)
    w = torch.randn((n, 24), generator=torch.Generator().manual_seed(8))

    def grads(fused, dtype, device):
        enc = TileEncoder(24, fused=fused)
        enc.load_state_dict(master.state_dict())
        enc = enc.to(device=device, dtype=dtype)
        x = torch.from_numpy(tiles).to(device=device, dtype=dtype)
        (enc(x) * w.to(device=device, dtype=dtype)).sum().backward()
        return {k: p.grad.double().cpu().numpy() for k, p in enc.named_parameters()}

    want = grads(False, torch.float64, "cpu")
    g_unfused, g_fused = grads(False, torch.float32, "cuda"), grads(True, torch.float32, "cuda")
    assert set(g_fused) == set(want) and len(want) == 7
    failed = []
    for name in ("embedding.weight", "tile_conv_1.weight", "tile_conv_1.bias"):
        assert np.abs(want[name]).max() > 0
        err = float(np.abs(g_fused[name] - want[name]).max())
        e_ref = float(np.abs(g_unfused[name] - want[name]).max())
        print(f"n={n} {kind} grad {name}: max|want| {np.abs(want[name]).max():.3e}  err / E_ref {err / e_ref:.3f}")
        try:
            within(f"n={n} {kind} grad {name}", g_fused[name], want[name], g_unfused[name])
        except AssertionError as e:
            failed.append(e)
    assert not failed, failed


# ---------------------------------------------------------------- c. determinism
def test_two_calls_give_identical_bits_at_1025_rows():
    n = 1025
    c = first(rows(), n)
    g = torch.randn(c.out_t.shape, generator=torch.Generator().manual_seed(9)).cuda()
    chunks = c.tile.n_chunks_for(n)
    a, ab = run_backward(c, c.idx_t, c.out_t, g, chunks)
    b, bb = run_backward(c, c.idx_t, c.out_t, g, chunks)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ab.view(torch.int32), bb.view(torch.int32))
    assert not a[61:].any() and a[60].any()
    bits = []
    for _ in range(2):
        table, bias = c.table_t.clone().requires_grad_(True), c.bias_t.clone().requires_grad_(True)
        c.tile.tile_conv1(c.x, table, bias).backward(g)
        bits.append((table.grad.view(torch.int32).clone(), bias.grad.view(torch.int32).clone()))
    assert torch.equal(bits[0][0], bits[1][0]) and torch.equal(bits[0][1], bits[1][1])
