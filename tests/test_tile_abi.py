"""The tile-encoder entry points of libnmmo_heads.so (include/nmmo_heads.h, SPEC.md §19) and
nmmo_amd/tile.py without a GPU: the constants match the header as a C compiler reads it, every
argument rule is refused with NMH_E_INVALID and a message naming the field (every call passes dummy
non-null pointers and n_rows <= 0, so a missing check shows as NMH_OK, never as a launch),
`tile_table` is the sum it says it is, and `TileEncoder(fused=False)` is the reference's module.
CPU only."""

import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from nmmo_amd import heads, tile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = 0x1000  # non-null, 16-byte aligned, never dereferenced


def test_constants_match_the_c_compiler():
    src = r"""
#include <stdio.h>
#include "nmmo_heads.h"
int main(void) {
  printf("%d %d %d %d %d %d %d %d %d %d\n", NMH_TILE_TILES, NMH_TILE_FEATURES, NMH_TILE_VALUES, NMH_TILE_TAPS,
         NMH_TILE_CHANNELS, NMH_TILE_OUT, NMH_TILE_FWD_ROWS, NMH_TILE_MAX_CHUNKS, NMH_TILE_F32, NMH_TILE_I16);
  return 0;
}
"""
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        with open(c, "w") as fh:
            fh.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [tile.TILES, tile.FEATURES, tile.VALUES, tile.TAPS, tile.CHANNELS, tile.OUT_SIDE ** 2,
                   tile.FWD_ROWS, tile.MAX_CHUNKS, tile.TILE_F32, tile.TILE_I16]
    assert got == [225, 3, 256, 9, 32, 169, 4, 64, 0, 1]
    assert tile.ROW == 675 and tile.CENTRE == 112 and tile.SIDE == 15


class Args:
    """Valid arguments with n_rows = 0; a test bends one of them."""

    def __init__(self):
        self.n_rows, self.tile, self.tile_stride, self.kind = 0, DUMMY, 675, tile.TILE_F32
        self.table = self.bias = self.out = self.idx_out = DUMMY
        self.idx = self.g_out = self.g_table_parts = self.g_bias_parts = DUMMY
        self.n_chunks = 1

    def forward(self):
        return heads.lib().nmh_tile_forward(self.n_rows, self.tile, self.tile_stride, self.kind, self.table, self.bias,
                                            self.out, self.idx_out, None)

    def backward(self):
        return heads.lib().nmh_tile_backward(self.n_rows, self.idx, self.out, self.g_out, self.n_chunks,
                                             self.g_table_parts, self.g_bias_parts, None)


def refused(a, fn, *words):
    rc = getattr(a, fn)()
    msg = heads.lib().nmh_last_error().decode()
    assert rc == heads.NMH_E_INVALID, (fn, rc, msg)
    assert msg.startswith(f"nmh_tile_{fn}:"), msg
    for w in words:
        assert w in msg, (fn, w, msg)


def test_valid_arguments_with_no_rows_are_a_no_op():
    a = Args()
    assert a.forward() == heads.NMH_OK and a.backward() == heads.NMH_OK
    a.idx_out = None  # optional
    a.kind, a.tile_stride, a.n_chunks = tile.TILE_I16, 23987, tile.MAX_CHUNKS
    assert a.forward() == heads.NMH_OK and a.backward() == heads.NMH_OK


@pytest.mark.parametrize("field", ["tile", "table", "bias", "out"])
def test_null_forward_arguments_are_refused(field):
    a = Args()
    setattr(a, field, None)
    refused(a, "forward", field, "NULL")


@pytest.mark.parametrize("field", ["idx", "out", "g_out", "g_table_parts", "g_bias_parts"])
def test_null_backward_arguments_are_refused(field):
    a = Args()
    setattr(a, field, None)
    refused(a, "backward", field, "NULL")


def test_bad_stride_kind_chunks_and_rows_are_refused():
    a = Args()
    a.tile_stride = 674
    refused(a, "forward", "tile_stride", "674")
    for kind in (2, -1):
        a = Args()
        a.kind = kind
        refused(a, "forward", "tile_kind", str(kind))
    for n_chunks in (0, -1, tile.MAX_CHUNKS + 1):
        a = Args()
        a.n_chunks = n_chunks
        refused(a, "backward", "n_chunks", str(n_chunks))
    a = Args()
    a.n_rows = -1
    refused(a, "forward", "n_rows", "-1")
    refused(a, "backward", "n_rows", "-1")


def test_unaligned_table_or_bias_is_refused():
    for field in ("table", "bias"):
        a = Args()
        setattr(a, field, DUMMY + 4)
        refused(a, "forward", field, "16-byte")
    for field in ("out", "g_out"):
        a = Args()
        setattr(a, field, DUMMY + 4)
        refused(a, "backward", field, "16-byte")
    a = Args()
    a.out = DUMMY + 4  # forward's out needs no alignment
    assert a.forward() == heads.NMH_OK


def test_n_chunks_is_a_function_of_the_row_count_within_the_limit():
    assert [tile.n_chunks_for(n) for n in (0, 1, 16, 17, 1024, 1025, 16384, 131072)] == [1, 1, 1, 2, 64, 64, 64, 64]


def test_tile_table_equals_explicit_loops():
    rng = np.random.default_rng(0)
    E = rng.standard_normal((768, 32))
    W = rng.standard_normal((32, 96, 3, 3))
    got = tile.tile_table(torch.from_numpy(E), torch.from_numpy(W)).numpy()
    assert got.shape == (3, 256, 9, 32)
    for f, v, k, o in [(0, 0, 0, 0), (2, 255, 8, 31), (1, 7, 5, 3), (2, 15, 4, 17), (0, 14, 2, 30), (1, 128, 7, 1)]:
        ky, kx = divmod(k, 3)
        want = sum(W[o][f * 32 + e][ky][kx] * E[f * 256 + v][e] for e in range(32))
        assert abs(got[f, v, k, o] - want) <= 1e-12 * max(1.0, abs(want)), (f, v, k, o)
    # and as a whole, against the same sum written with numpy
    want = np.einsum("ofeyx,fve->fvyxo", W.reshape(32, 3, 32, 3, 3), E.reshape(3, 256, 32)).reshape(3, 256, 9, 32)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    t = tile.tile_table(torch.from_numpy(E).requires_grad_(True), torch.from_numpy(W))
    assert t.requires_grad and t.is_contiguous()


def reference_forward(enc, tile_in):
    """baseline_policy.py:95-112 restated on the module's parameters (it edits `tile_in` in place)."""
    tile_in[:, :, :2] -= tile_in[:, 112:113, :2].clone()
    tile_in[:, :, :2] += 7
    t = F.embedding(tile_in.long().clip(0, 255) + torch.tensor([0, 256, 512]), enc.embedding.weight)
    agents, tiles, features, embed = t.shape
    t = t.view(agents, tiles, features * embed).transpose(1, 2).view(agents, features * embed, 15, 15)
    t = F.relu(F.conv2d(t, enc.tile_conv_1.weight, enc.tile_conv_1.bias))
    t = F.relu(F.conv2d(t, enc.tile_conv_2.weight, enc.tile_conv_2.bias))
    t = t.contiguous().view(agents, -1)
    return F.relu(F.linear(t, enc.tile_fc.weight, enc.tile_fc.bias))


def sample_tiles(n, rng):
    """[n, 225, 3] float32 tiles: windows at random map positions, row 0 all zero (an agent not in
    the realm), row 1 centred on map coordinate 0 (the window's coordinates run from -7), row 2 junk
    that clips at 0 and at 255, with materials 0, 15, 255 and beyond."""
    yy, xx = np.meshgrid(np.arange(15), np.arange(15), indexing="ij")
    t = np.zeros((n, 225, 3), dtype=np.float32)
    for r in range(n):
        r0, c0 = rng.integers(0, 160, 2)
        t[r, :, 0], t[r, :, 1] = (r0 + yy).ravel(), (c0 + xx).ravel()
        t[r, :, 2] = rng.integers(0, 16, 225)
    t[0] = 0
    if n > 1:
        t[1, :, 0], t[1, :, 1] = (yy - 7).ravel(), (xx - 7).ravel()
    if n > 2:
        t[2] = rng.integers(-400, 400, (225, 3))
        t[2, :4, 2] = [0, 15, 255, 300]
    return t


def test_unfused_encoder_equals_the_reference_and_leaves_its_input_unchanged():
    torch.manual_seed(1)
    enc = tile.TileEncoder(48)
    x = torch.from_numpy(sample_tiles(5, np.random.default_rng(2)))
    keep = x.clone()
    got = enc(x)
    assert torch.equal(x, keep)
    want = reference_forward(enc, x.clone())
    assert got.shape == (5, 48) and torch.equal(got, want)
    # the same rows as the Tile section of wider flat rows, and as int16
    wide = torch.zeros((5, 700))
    wide[:, 20:695] = keep.reshape(5, 675)
    assert torch.equal(enc(wide, 20), want)
    assert torch.equal(enc(keep.to(torch.int16)), want)
    assert torch.equal(tile.tile_indices(keep), tile.tile_indices(keep.to(torch.int16)))


def test_state_dict_keys_and_shapes_are_the_references():
    for fused in (False, True):
        sd = tile.TileEncoder(256, fused=fused).state_dict()
        assert {k: tuple(v.shape) for k, v in sd.items()} == {
            "embedding.weight": (768, 32), "tile_conv_1.weight": (32, 96, 3, 3), "tile_conv_1.bias": (32,),
            "tile_conv_2.weight": (8, 32, 3, 3), "tile_conv_2.bias": (8,), "tile_fc.weight": (256, 968),
            "tile_fc.bias": (256,)}
    a, b = tile.TileEncoder(32), tile.TileEncoder(32, fused=True)
    b.load_state_dict(a.state_dict())
    a.load_state_dict(b.state_dict())


def test_host_tensors_are_refused_without_a_fallback():
    enc = tile.TileEncoder(32, fused=True)
    x = torch.zeros((2, 225, 3))
    with pytest.raises(heads.HeadsError, match="GPU"):
        tile.tile_conv1(x, tile.tile_table(enc.embedding.weight, enc.tile_conv_1.weight), enc.tile_conv_1.bias)
    with pytest.raises(heads.HeadsError):
        enc(x)


def test_tile_agent_keeps_the_stand_ins_call_convention_on_the_cpu():
    from nmmo_amd import layout
    from nmmo_amd.trainer import TileMaskedAgent

    torch.manual_seed(0)
    agent = TileMaskedAgent(16, hidden=32)
    assert not agent.tile_encoder.fused and not agent.fused_heads
    obs = torch.zeros((3, layout.obs_elems(16)))
    obs[:, :sum(agent.dims)] = 1.0
    a, logp, ent, value = agent(obs)
    assert a.shape == (3, len(agent.dims)) and logp.shape == ent.shape == (3,) and value.shape == (3, 1)
    assert {n.split(".")[0] for n, _ in agent.named_parameters()} == {"tile_encoder", "encoder", "actor", "value"}
