"""nmh_tile2_forward (SPEC.md §22) at the C4 row count and at an offset past 2^31 elements, with the
two constructions of tests/test_gpu_learner_fullsize.py (its buffer, pattern rows, geometry and
comparisons are imported, not copied). Forward only.

A. nine rows as an `as_strided` view of the 12.6 GB flat buffer whose stride is chosen so that row
   6's Tile section contains element offset 2^31 and rows 7 and 8 lie wholly past it: `tile_conv12`
   and the C call on the view equal the same calls on the compact copy of the rows, bit for bit; the
   wrapper hands the view's own pointer on and allocates its output and nothing else.
B. one launch over 131,072 rows holding pattern row r % 37: out2 (507 MB) and idx (88 MB) lie inside
   canary margins, output row r equals row r % 37 of the 37-row call, and the buffer still holds
   the tiling afterwards.

Index audit of the new kernels, read before the first full-size run (every line is 64-bit):
  tile_enc  nmh_tile2_forward_kernel   row0 = (int64_t)blockIdx.x * kFwd2Rows; n = row0 + r (int64_t);
                                       tile + n * tile_stride (tile_stride int64_t);
                                       idx_out + n * kRowIdx; out2 + n * kRowOut2 + (4 * g) * kP2 + p2
                                       (the added terms are below 968); s_idx / s_a1 offsets are LDS, below 5,408
  tile_enc  nmh_tile2_backward_kernel  lo = (int64_t)blockIdx.x * rows_per_part, hi int64_t, n int64_t;
                                       idx + n * kRowIdx; out2 + n * kRowOut2; g_out2 + n * kRowOut2;
                                       dz1 + n * kRowOut; g_w2_parts + (int64_t)blockIdx.x * kW2;
                                       g_bias2_parts + (int64_t)blockIdx.x * kO2
  tile_enc  nmh_tile_backward_kernel   (gated instantiation) unchanged: out + n * kRowOut is formed but never read
  host      grids: (n_rows + 3) / 4 = 32,768 and n_w2_parts <= 1,024 workgroups as unsigned;
            rows_per_part = ceil(n_rows / n_w2_parts) in int64_t, then int (at most n_rows)
  wrapper   `_tile_arg` passes `stride(0)` as a Python int into an int64_t parameter (ctypes c_int64)
No defect was found by reading.
"""

from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.conftest import gpu_available
from tests.test_gpu_learner_fullsize import (DEV, F32, GEO, K, ROWS, SEL, T_LEN, T_OFF, U8, Guarded, big,  # noqa: F401
                                             bits, grows, launched, note_memory, patterns, ptr, same, stream, tiled,
                                             tiling_holds, view_of)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

_weights = {}


def weights():
    """tile_conv_2's weight and bias, general values; the table and bias1 are the patterns' own."""
    if not _weights:
        rng = np.random.default_rng(2231)
        _weights.update(w2=torch.from_numpy((rng.standard_normal((8, 32, 3, 3)) / 8).astype(np.float32)).to(DEV),
                        bias2=torch.from_numpy(rng.standard_normal(8).astype(np.float32)).to(DEV))
    return _weights["w2"], _weights["bias2"]


def run_tile2(rows, x, measure):
    from nmmo_amd import heads, tile

    n = rows.shape[0]
    w2, bias2 = weights()
    sec = rows[:, T_OFF:T_OFF + T_LEN]
    arg, stride, kind = tile._tile_arg(sec, None)
    assert arg.data_ptr() == sec.data_ptr() == rows.data_ptr() + T_OFF * rows.element_size() and stride == rows.stride(0)
    tab = x.table.clone().requires_grad_(True)
    with grows(measure, "tile_conv12 with grad", ((n, 8, 11, 11), F32), ((n, 225, 3), U8)):
        out = tile.tile_conv12(sec, tab, x.bias, w2, bias2)
    with torch.no_grad(), grows(measure, "tile_conv12 without grad", ((n, 8, 11, 11), F32)):
        out_b = tile.tile_conv12(sec, x.table, x.bias, w2, bias2)
    out_c = torch.empty_like(out_b)
    idx = torch.empty((n, 225, 3), dtype=U8, device=DEV)
    heads.check(heads.lib().nmh_tile2_forward(n, ptr(arg), stride, kind, ptr(x.table), ptr(x.bias), ptr(w2), ptr(bias2),
                                              ptr(out_c), ptr(idx), stream()), "nmh_tile2_forward")
    torch.cuda.synchronize()
    return [out.detach(), out_b, out_c, idx]


def test_a_tile_conv12_on_a_view_that_straddles_element_offset_2_to_the_31(big):  # noqa: F811
    buf, state = big
    P = patterns(True)
    x = P.inputs(sel=SEL)
    compact = P.rows[SEL]
    state.tiled = False
    geo = GEO["Tile", "e31"]
    v = view_of(buf.view(-1), geo, compact)
    first = geo.row * geo.stride + T_OFF  # element offsets of the straddling row's section
    assert first < (1 << 31) <= first + T_LEN - 1 and (geo.row + 1) * geo.stride > (1 << 31)
    got, want = run_tile2(v, x, True), run_tile2(compact, x, False)
    note_memory()
    same(got, want)
    assert float(want[0].max()) > 0 and int(want[3].max()) == 255
    assert torch.equal(bits(v), bits(compact)), "the rows were written"


def raw_tile2(rows, n, x, after):
    from nmmo_amd import heads, tile

    g = Guarded()
    w2, bias2 = weights()
    arg, stride, kind = tile._tile_arg(rows[:, T_OFF:T_OFF + T_LEN], None)
    assert arg.data_ptr() == rows.data_ptr() + 4 * T_OFF and stride == rows.stride(0)
    out2, idx = g.new((n, 8, 11, 11)), g.new((n, 225, 3), U8)
    launched(after, heads.lib().nmh_tile2_forward(n, ptr(arg), stride, kind, ptr(x.table), ptr(x.bias), ptr(w2), ptr(bias2),
                                                  ptr(out2), ptr(idx), stream()), "nmh_tile2_forward")
    g.check()
    return [out2, idx]


def test_b_tile2_forward_over_every_row(tiled):  # noqa: F811
    buf, P = tiled
    keep = P.rows.clone()

    def small_unchanged(name):
        assert torch.equal(bits(P.rows), bits(keep)), f"{name} changed the 37 rows"

    def big_unchanged(name):
        assert tiling_holds(buf, P.rows), f"{name} changed the obs buffer"

    x = SimpleNamespace(**P.shared)  # the table and bias1: no per-row inputs
    ref = raw_tile2(P.rows, K, x, small_unchanged)
    got = raw_tile2(buf, ROWS, x, big_unchanged)
    assert got[0].numel() * 4 == 507_510_784
    assert float(ref[0].max()) > 0 and bool((ref[0] == 0).any())
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a.shape[0] == ROWS and b.shape[0] == K and a.shape[1:] == b.shape[1:]
        assert tiling_holds(a, b), f"output {i}: a row differs from its pattern row's"
