"""nmh_tile2_forward / nmh_tile2_backward of libnmmo_heads.so (include/nmmo_heads.h, SPEC.md §22)
and `tile.tile_conv12` / `TileEncoder(fused_conv2=True)` without a GPU: the new constants match the
header as a C compiler reads it, every argument rule is refused with NMH_E_INVALID and a message
naming the field (every call passes dummy non-null pointers and n_rows <= 0, so a missing check
shows as NMH_OK, never as a launch), `n_w2_parts_for` is a capped monotone function of N, and the
numpy restatements of §22 that the GPU tests compare the kernels with (`spec2_forward` in float32,
term by term in §22's order; `spec2_backward` in float64) are what they say they are. CPU only."""

import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from nmmo_amd import heads, tile
from tests.test_tile_abi import sample_tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = 0x1000  # non-null, 16-byte aligned, never dereferenced
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


def spec_a1(idx, table, bias1):
    """§19's forward in float32, one addition at a time in the order it fixes: a1 [N, 32, 13, 13]."""
    n = idx.shape[0]
    win = idx.reshape(n, 15, 15, 3)
    z = np.broadcast_to(bias1.astype(F32)[None, None, None, :], (n, 13, 13, 32)).copy()
    for ky in range(3):
        for kx in range(3):
            for f in range(3):
                z = (z + table[f][:, ky * 3 + kx, :][win[:, ky:ky + 13, kx:kx + 13, f]]).astype(F32)
    return np.ascontiguousarray(np.maximum(z, F32(0.0)).transpose(0, 3, 1, 2))


def spec2_forward(a1, w2, bias2):
    """§22's second convolution in float32: z = b2, then one multiply and one add per term in the
    order c, ky, kx: out2 [N, 8, 11, 11]."""
    n = a1.shape[0]
    a1, w2 = a1.astype(F32), w2.astype(F32)
    z = np.broadcast_to(bias2.astype(F32)[None, :, None, None], (n, 8, 11, 11)).copy()
    for c in range(32):
        for ky in range(3):
            for kx in range(3):
                term = (w2[None, :, c, ky, kx, None, None] * a1[:, None, c, ky:ky + 11, kx:kx + 11]).astype(F32)
                z = (z + term).astype(F32)
    return np.maximum(z, F32(0.0))


def spec2_backward(idx, a1, out2, g_out2, w2):
    """§22's gradients in float64: (g_table [3, 256, 9, 32], g_bias1 [32], g_w2 [8, 32, 3, 3],
    g_bias2 [8], dz1 [N, 32, 13, 13])."""
    n = idx.shape[0]
    a, w = a1.astype(np.float64), w2.astype(np.float64)
    dz2 = np.where(out2 > 0, g_out2, 0).astype(np.float64)
    g_w2, dz1 = np.zeros((8, 32, 3, 3)), np.zeros((n, 32, 13, 13))
    for ky in range(3):
        for kx in range(3):
            g_w2[:, :, ky, kx] = np.einsum("noyx,ncyx->oc", dz2, a[:, :, ky:ky + 11, kx:kx + 11])
            dz1[:, :, ky:ky + 11, kx:kx + 11] += np.einsum("noyx,oc->ncyx", dz2, w[:, :, ky, kx])
    dz1 *= a > 0
    win = idx.reshape(n, 15, 15, 3)
    flat = dz1.transpose(0, 2, 3, 1).reshape(-1, 32)
    g_table = np.zeros((3, 256, 9, 32))
    for ky in range(3):
        for kx in range(3):
            for f in range(3):
                part = np.zeros((256, 32))
                np.add.at(part, win[:, ky:ky + 13, kx:kx + 13, f].reshape(-1), flat)
                g_table[f, :, ky * 3 + kx, :] = part
    return g_table, flat.sum(0), g_w2, dz2.sum((0, 2, 3)), dz1


def exact_state(seed=3, input_size=32):
    """A TileEncoder state_dict whose partial sums are exact in any order: embedding weights from
    {-1, 0, 1}; tile_conv_1.weight, both biases and tile_conv_2.weight from {-2..2}/2. Then every
    table entry is a multiple of 1/2 with |T| <= 32, |a1| <= 1 + 27 x 32 = 865 in multiples of 1/2,
    and |z2| <= 1 + 288 x 865 < 2.5e5 in multiples of 1/4: far below 2^24 of their unit."""
    g = torch.Generator().manual_seed(seed)
    sd = tile.TileEncoder(input_size).state_dict()
    sd["embedding.weight"] = torch.randint(-1, 2, sd["embedding.weight"].shape, generator=g).float()
    for k in ("tile_conv_1.weight", "tile_conv_1.bias", "tile_conv_2.weight", "tile_conv_2.bias"):
        sd[k] = torch.randint(-2, 3, sd[k].shape, generator=g) / 2.0
    for k in ("tile_fc.weight", "tile_fc.bias"):  # general, and the same on every call
        sd[k] = torch.randn(sd[k].shape, generator=g) / 32.0
    return sd


# ---------------------------------------------------------------- constants
def test_new_constants_match_the_c_compiler():
    src = r"""
#include <stdio.h>
#include "nmmo_heads.h"
int main(void) {
  printf("%d %d %d %d %d\n", NMH_TILE2_CHANNELS, NMH_TILE2_OUT, NMH_TILE2_FWD_ROWS, NMH_TILE2_MAX_PARTS,
         NMH_TILE_MAX_CHUNKS);
  return 0;
}
"""
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        with open(c, "w") as fh:
            fh.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [tile.CHANNELS2, tile.OUT2_SIDE ** 2, tile.FWD2_ROWS, tile.MAX_W2_PARTS, tile.MAX_CHUNKS]
    assert got == [8, 121, 4, 1024, 64]


# ---------------------------------------------------------------- argument rules
FWD_PTRS = ["tile", "table", "bias1", "w2", "bias2", "out2"]
BWD_PTRS = ["idx", "out2", "g_out2", "table", "bias1", "w2", "dz1_scratch", "g_table_parts", "g_bias1_parts",
            "g_w2_parts", "g_bias2_parts"]


class Args:
    """Valid arguments with n_rows = 0; a test bends one of them."""

    def __init__(self):
        self.n_rows, self.tile_stride, self.kind = 0, 675, tile.TILE_F32
        for name in FWD_PTRS + BWD_PTRS + ["idx_out"]:
            setattr(self, name, DUMMY)
        self.n_table_chunks = self.n_w2_parts = 1

    def forward(self):
        return heads.lib().nmh_tile2_forward(self.n_rows, self.tile, self.tile_stride, self.kind, self.table, self.bias1,
                                             self.w2, self.bias2, self.out2, self.idx_out, None)

    def backward(self):
        return heads.lib().nmh_tile2_backward(self.n_rows, self.idx, self.out2, self.g_out2, self.table, self.bias1,
                                              self.w2, self.n_table_chunks, self.n_w2_parts, self.dz1_scratch,
                                              self.g_table_parts, self.g_bias1_parts, self.g_w2_parts,
                                              self.g_bias2_parts, None)


def refused(a, fn, *words):
    rc = getattr(a, fn)()
    msg = heads.lib().nmh_last_error().decode()
    assert rc == heads.NMH_E_INVALID, (fn, rc, msg)
    assert msg.startswith(f"nmh_tile2_{fn}:"), msg
    for w in words:
        assert w in msg, (fn, w, msg)


def test_valid_arguments_with_no_rows_are_a_no_op():
    a = Args()
    assert a.forward() == heads.NMH_OK and a.backward() == heads.NMH_OK
    a.idx_out = None  # optional
    a.kind, a.tile_stride = tile.TILE_I16, 23987
    a.n_table_chunks, a.n_w2_parts = tile.MAX_CHUNKS, tile.MAX_W2_PARTS
    assert a.forward() == heads.NMH_OK and a.backward() == heads.NMH_OK
    a.out2 = a.g_out2 = DUMMY + 4  # out2 and g_out2 need no alignment beyond a float's
    assert a.forward() == heads.NMH_OK and a.backward() == heads.NMH_OK


@pytest.mark.parametrize("field", FWD_PTRS)
def test_null_forward_arguments_are_refused(field):
    a = Args()
    setattr(a, field, None)
    refused(a, "forward", field, "NULL")


@pytest.mark.parametrize("field", BWD_PTRS)
def test_null_backward_arguments_are_refused(field):
    a = Args()
    setattr(a, field, None)
    refused(a, "backward", field, "NULL")


def test_bad_stride_kind_counts_and_rows_are_refused():
    a = Args()
    a.tile_stride = 674
    refused(a, "forward", "tile_stride", "674")
    for kind in (2, -1):
        a = Args()
        a.kind = kind
        refused(a, "forward", "tile_kind", str(kind))
    for n in (0, -1, tile.MAX_CHUNKS + 1):
        a = Args()
        a.n_table_chunks = n
        refused(a, "backward", "n_table_chunks", str(n))
    for n in (0, -1, tile.MAX_W2_PARTS + 1):
        a = Args()
        a.n_w2_parts = n
        refused(a, "backward", "n_w2_parts", str(n))
    a = Args()
    a.n_rows = -1
    refused(a, "forward", "n_rows", "-1")
    refused(a, "backward", "n_rows", "-1")


def test_unaligned_weights_and_scratch_are_refused():
    for field in ("table", "bias1", "w2", "bias2"):
        a = Args()
        setattr(a, field, DUMMY + 4)
        refused(a, "forward", field, "16-byte")
    for field in ("table", "bias1", "w2", "dz1_scratch"):
        a = Args()
        setattr(a, field, DUMMY + 4)
        refused(a, "backward", field, "16-byte")


# ---------------------------------------------------------------- tile.py
def test_n_w2_parts_is_a_capped_monotone_function_of_the_row_count():
    got = [tile.n_w2_parts_for(n) for n in (0, 1, 4, 5, 37, 1024, 4096, 4097, 16384, 131072)]
    assert got == [1, 1, 1, 2, 10, 256, 1024, 1024, 1024, 1024]
    all_n = [tile.n_w2_parts_for(n) for n in range(0, 5000)]
    assert min(all_n) >= 1 and max(all_n) == tile.MAX_W2_PARTS
    assert all(b >= a for a, b in zip(all_n, all_n[1:]))
    assert all(p <= max(1, n) for n, p in enumerate(all_n))  # never more parts than rows


def test_fused_conv2_needs_the_fused_path():
    with pytest.raises(ValueError, match="fused=True"):
        tile.TileEncoder(32, fused=False, fused_conv2=True)
    enc = tile.TileEncoder(32, fused=True, fused_conv2=True)
    assert enc.fused and enc.fused_conv2 and not tile.TileEncoder(32, fused=True).fused_conv2


def test_state_dict_keys_and_shapes_are_the_unfused_modules():
    want = {k: tuple(v.shape) for k, v in tile.TileEncoder(256).state_dict().items()}
    assert len(want) == 7 and want["tile_conv_2.weight"] == (8, 32, 3, 3) and want["tile_fc.weight"] == (256, 968)
    enc = tile.TileEncoder(256, fused=True, fused_conv2=True)
    assert {k: tuple(v.shape) for k, v in enc.state_dict().items()} == want
    plain = tile.TileEncoder(256)
    enc.load_state_dict(plain.state_dict())
    plain.load_state_dict(enc.state_dict())


def test_host_tensors_are_refused_without_a_fallback():
    enc = tile.TileEncoder(32, fused=True, fused_conv2=True)
    x = torch.zeros((2, 225, 3))
    table = tile.tile_table(enc.embedding.weight, enc.tile_conv_1.weight)
    with pytest.raises(heads.HeadsError, match="GPU"):
        tile.tile_conv12(x, table, enc.tile_conv_1.bias, enc.tile_conv_2.weight, enc.tile_conv_2.bias)
    with pytest.raises(heads.HeadsError):
        enc(x)


def test_tile_agent_passes_the_flag_on_and_keeps_it_off_by_default():
    from nmmo_amd.trainer import TileMaskedAgent

    assert not TileMaskedAgent(16, hidden=32).tile_encoder.fused_conv2
    assert not TileMaskedAgent(16, hidden=32, fused_tile=True).tile_encoder.fused_conv2
    agent = TileMaskedAgent(16, hidden=32, fused_tile=True, fused_tile_conv2=True)
    assert agent.tile_encoder.fused and agent.tile_encoder.fused_conv2
    with pytest.raises(ValueError):
        TileMaskedAgent(16, hidden=32, fused_tile_conv2=True)


# ---------------------------------------------------------------- the restatements
def test_restatement_agrees_with_float64_within_float32_error_for_general_weights():
    """The second convolution on one float32 a1, restated in float32 and by torch in float64. A chain
    of one product and one addition per term over 288 terms and the bias has a relative error of at
    most gamma_290 = 290 u / (1 - 290 u), u = 2^-24, of the sum of the absolute values of its terms
    (Higham, Accuracy and Stability of Numerical Algorithms, §3.1); the ReLU does not enlarge it."""
    rng = np.random.default_rng(5)
    idx = spec_indices(sample_tiles(5, rng))
    a1 = spec_a1(idx, rng.standard_normal((3, 256, 9, 32)).astype(F32), rng.standard_normal(32).astype(F32))
    w2, b2 = rng.standard_normal((8, 32, 3, 3)).astype(F32), rng.standard_normal(8).astype(F32)
    got = spec2_forward(a1, w2, b2)
    assert got.dtype == F32 and got.shape == (5, 8, 11, 11) and (got > 0).any() and (got == 0).any()
    a64, w64, b64 = (torch.from_numpy(t).double() for t in (a1, w2, b2))
    want = F.relu(F.conv2d(a64, w64, b64)).numpy()
    size = (F.conv2d(a64.abs(), w64.abs()) + b64.abs()[None, :, None, None]).numpy()
    u = 2.0 ** -24
    bound = 290 * u / (1 - 290 * u) * size
    err = np.abs(got.astype(np.float64) - want)
    print(f"max err {err.max():.3e}, max bound {bound.max():.3e}, max err / bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert err.max() > 0  # float32 did round: the two are not the same computation


def test_restatement_equals_the_float64_chain_bit_for_bit_on_exact_weights():
    """`exact_state`: every partial sum of either chain is exact, so the float32 restatement of §19
    and §22 equals the unfused module's float64 chain, value for value."""
    enc = tile.TileEncoder(32)
    enc.load_state_dict(exact_state())
    tiles = sample_tiles(5, np.random.default_rng(6))
    with torch.no_grad():
        table = tile.tile_table(enc.embedding.weight, enc.tile_conv_1.weight).numpy()
        assert np.array_equal(table * 2, np.round(table * 2)) and np.abs(table).max() <= 32
        a1 = spec_a1(spec_indices(tiles), table, enc.tile_conv_1.bias.numpy())
        got = spec2_forward(a1, enc.tile_conv_2.weight.numpy(), enc.tile_conv_2.bias.numpy())
        enc64 = tile.TileEncoder(32).double()
        enc64.load_state_dict(exact_state())
        a1_64 = enc64.conv1(torch.from_numpy(tiles).double())
        want = F.relu(enc64.tile_conv_2(a1_64)).numpy()
        want32 = F.relu(enc.tile_conv_2(enc.conv1(torch.from_numpy(tiles)))).numpy()
    assert np.abs(a1).max() <= 865 and np.array_equal(a1.astype(np.float64), a1_64.numpy())
    assert want.max() > 100 and (want == 0).any()
    assert np.array_equal(got.astype(np.float64), want)
    assert np.array_equal(want32.astype(np.float64), want)  # the float32 torch chain too


def test_backward_restatement_equals_torch_autograd_in_float64():
    rng = np.random.default_rng(7)
    tiles = sample_tiles(4, rng)
    idx = spec_indices(tiles)
    table = torch.from_numpy(rng.standard_normal((3, 256, 9, 32))).requires_grad_(True)
    b1 = torch.from_numpy(rng.standard_normal(32)).requires_grad_(True)
    w2 = torch.from_numpy(rng.standard_normal((8, 32, 3, 3))).requires_grad_(True)
    b2 = torch.from_numpy(rng.standard_normal(8)).requires_grad_(True)
    win = torch.from_numpy(idx.astype(np.int64)).reshape(4, 15, 15, 3)
    z = b1[None, None, None, :].expand(4, 13, 13, 32)
    for ky in range(3):
        for kx in range(3):
            for f in range(3):
                z = z + table[f][:, ky * 3 + kx, :][win[:, ky:ky + 13, kx:kx + 13, f]]
    a1 = F.relu(z.permute(0, 3, 1, 2))
    out2 = F.relu(F.conv2d(a1, w2, b2))
    g = torch.from_numpy(rng.standard_normal((4, 8, 11, 11)))
    out2.backward(g)
    got = spec2_backward(idx, a1.detach().numpy(), out2.detach().numpy(), g.numpy(), w2.detach().numpy())
    for name, a, b in zip(("g_table", "g_bias1", "g_w2", "g_bias2"), got, (table.grad, b1.grad, w2.grad, b2.grad)):
        np.testing.assert_allclose(a, b.numpy(), rtol=1e-12, atol=1e-12, err_msg=name)
