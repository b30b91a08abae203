"""The decoder kernels (nmmo_amd/decoder.py, csrc/decoder.hip, SPEC.md §23) where the row index times
the row stride no longer fits 32 bits: fashion A of tests/test_gpu_learner_fullsize.py, nine-row
`as_strided` views of one large buffer, with that module's geometry, pattern rows, fixtures and
comparison unchanged (tests/test_learner_fullsize_geometry.py checks the geometry on the CPU). Forward
(given and sampled) and backward on the view must equal the compact call bit for bit, the wrapper must
hand the view's own pointers on, and a call may allocate its outputs and nothing else (`grows`).

  Market e31   float32 rows; row 6's Market section contains element offset 2^31, rows 7 and 8 lie past
               it: the row-times-stride product of every set and of the mask passes 2^31
  mask e31     the same with the boundary inside row 6's mask prefix
  Market i16   int16 rows and a uint8 mask, the boundary in the last row's Market section and mask: the
               other element and mask instantiation (the product itself stays below 2^31 there)

The 131,072-row pass (fashion B) is not part of this module.

Index audit of decoder.hip, read before the first run (r: row; every line is 64-bit unless it says LDS):
  both kernels   r = (int64_t)blockIdx.x * (blockDim.x >> 6) + w; the grid is (n + rpb - 1) / rpb unsigned
  both kernels   pq[r * pl.n_ptr * kSlot + i] (r int64_t); mbase = r * ms + off (r, ms int64_t), + i < dims[k]
  set_of         base + (r / share) * stride: int64_t r, int32 share, int64_t stride; the cast to T* is first
  forward        dense + r * ds + src; cand + (int64_t)j * item_dev::kC (load_item); stage_rows:
                 set[(int64_t)(list[i0 + k] & 4095) * kC + c]
  tile_heads     actions_in[r * n_heads + k]; q = r * n_heads + k; philox(row_base + (uint32_t)r, ..): 32-bit by definition
  backward       hq = r * pl.n_heads + k; dense + r * ds + src; g_dense + r * gds + src (gds int64_t);
                 cand[(int64_t)m.list[i0 + u] * kC + col]; g_pq[(r * pl.n_ptr + src) * kSlot + f]
  LDS            staged + (size_t)w * wave_bytes; s[off + j], j <= R, off + R < total; pq slot src * 40 + 0..35 <
                 n_ptr * 40; list[i], i < cnt <= R <= U's 2 R bytes; rows[e], e < 64 * 31, behind the largest
                 entity list; sg[i], i < cnt <= R < total. The host sizes wave_bytes from the same plan.
  decoder.py     strides go from `stride(0)` as Python ints into int64_t fields (ctypes c_int64) of
                 NmhDecoderSets and into the int64_t mask_stride / dense_stride arguments
No defect was found by reading."""

import numpy as np
import pytest
import torch

from tests.conftest import gpu_available
from tests.test_gpu_learner_fullsize import (DEV, DIMS, E_LEN, E_OFF, F32, I32, I_LEN, I_OFF, M_LEN, M_OFF, N_A,  # noqa: F401
                                             OFFSET, SEED, TOTAL, a_compare, a_views, big, grows, small)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

HEAD_SET = [-1, 0, 2, 1, 1, 0, -1, 0, -1, 1, -1, 1]  # sets: Entity, Inventory, Market
N_DENSE = sum(d for d, s in zip(DIMS, HEAD_SET) if s < 0)
N_PTR = sum(s >= 0 for s in HEAD_SET)


def queries():
    rng = np.random.default_rng(77)
    pq = rng.standard_normal((N_A, N_PTR, 40)).astype(np.float32)
    for p, k in enumerate(k for k, s in enumerate(HEAD_SET) if s >= 0):
        if HEAD_SET[k] == 0:  # raw entity columns reach 32,767
            pq[:, p, 0], pq[:, p, 6:35] = pq[:, p, 0] * 2.0 ** -12, pq[:, p, 6:35] * 2.0 ** -12
        else:
            pq[:, p, 20:32] *= 2.0 ** -4
    dense = rng.standard_normal((N_A, N_DENSE)).astype(np.float32)
    return torch.from_numpy(dense).to(DEV), torch.from_numpy(pq).to(DEV)


def run_decoder(rows, mask_rows, x, measure):
    from nmmo_amd import item, player
    from nmmo_amd.decoder import decoder_heads_full

    n, H = rows.shape[0], len(DIMS)
    secs = [rows[:, E_OFF:E_OFF + E_LEN], rows[:, I_OFF:I_OFF + I_LEN], rows[:, M_OFF:M_OFF + M_LEN]]
    for sec, arg, R in zip(secs, (player._ent_arg, item._item_arg, item._item_arg), (100, 12, 1024)):
        got, stride, r_, _ = arg(sec, R)
        assert got.data_ptr() == sec.data_ptr() and (stride, r_) == (rows.stride(0), R)  # read in place
    sets = [(secs[0], "entity"), (secs[1], "item"), (secs[2], "item")]
    five = [((n, H), I32), ((n,), F32), ((n,), F32), ((n, H), F32), ((n, H), F32)]
    dense, pq = queries()
    d, q = dense.clone().requires_grad_(True), pq.clone().requires_grad_(True)
    with grows(measure, "decoder_heads forward", *five):
        _, lp, ent, lse, hent = decoder_heads_full(d, q, sets, HEAD_SET, mask_rows, DIMS, x.actions32)
    with grows(measure, "decoder_heads backward", (d.shape, F32), (q.shape, F32)):
        g = torch.autograd.grad([lp, ent], [d, q], [x.glp, x.gen])
    with grows(measure, "decoder_heads sampled", *five):
        s = decoder_heads_full(dense, pq, sets, HEAD_SET, mask_rows, DIMS, seed=SEED, offset=OFFSET)
    assert float(g[1].abs().max()) > 0
    return [lp.detach(), ent.detach(), lse, hent, *g, *s]


@pytest.mark.parametrize("name,kind", [("Market", "e31"), ("mask", "e31"), ("Market", "i16")])
def test_a_decoder_heads_on_a_straddling_view(name, kind, big, small):
    v, vm, compact, cm, x = a_views(kind, name, big, small)
    if name == "mask" and kind == "e31":
        assert v is vm and v.stride(0) * 6 < (1 << 31) <= v.stride(0) * 6 + TOTAL
    a_compare(run_decoder, v, vm, compact, cm, x)
