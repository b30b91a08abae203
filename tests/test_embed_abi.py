"""The embedded-set entry points of libnmmo_heads.so (include/nmmo_heads.h, SPEC.md §25) and
nmmo_amd/embed.py without a GPU: the constants match the header as a C compiler reads it; header,
`heads.SYMBOLS` and the ctypes declarations agree; every argument rule is refused with NMH_E_INVALID
and the library's message naming the field (every call passes dummy non-null pointers and n = 0, so
a missing check shows as NMH_OK, never as a launch); `embed_features_ref` equals a numpy restatement
bit for bit on the clip edges; and in float64 `pointer_query`'s pq and the pool from counts and sums
reproduce q . fc(feat) and mean_j fc(feat_j) of the materialised chain. CPU only."""

import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from nmmo_amd import _sets, abi, embed, heads, item, player
from nmmo_amd.embed import ENTITY, ITEM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = 0x1000  # non-null, 16-byte aligned, never dereferenced
KINDS = [ENTITY, ITEM]
NEW = ["nmh_embed_features", "nmh_embed_logits", "nmh_embed_logits_backward"]


def test_constants_match_the_c_compiler():
    src = r"""
#include <stdio.h>
#include "nmmo_heads.h"
int main(void) {
  printf("%d %d %d %d %d %d %d %d %d\n", NMH_EMBED_ENTITY, NMH_EMBED_ITEM, NMH_EMBED_BINS, NMH_EMBED_ENTITY_QUERY,
         NMH_EMBED_ITEM_QUERY, NMH_PLAYER_MAX_ROWS, NMH_ITEM_MAX_ROWS, NMH_ELEM_F32, NMH_ELEM_I16);
  return 0;
}
"""
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        with open(c, "w") as fh:
            fh.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [ENTITY.code, ITEM.code, embed.BINS, ENTITY.query, ITEM.query, ENTITY.max_rows, ITEM.max_rows,
                   _sets.ELEM_F32, _sets.ELEM_I16]
    assert got == [0, 1, 256, 1052, 528, 256, 1024, 0, 1]


def test_the_descriptors_are_the_reference_constructors_values():
    F = abi.F
    assert (ENTITY.cols, ENTITY.D, ENTITY.C, ENTITY.features, ENTITY.bias) == (31, 4, 27, 155, 1051)
    assert ENTITY.dcols == (F["id"], F["npc_type"], F["attacker_id"], F["message"]) == (0, 1, 8, 10)
    assert ENTITY.doffs == (0, 256, 512, 768)
    assert ENTITY.ccols == tuple(c for c in range(31) if c not in ENTITY.dcols)
    assert ENTITY.cdivs == (256, 256, 100, 1024, 3, 50, 1024, 100, 100, 100, 100) + (10, 100) * 7 + (100, 10)
    assert ENTITY.cdivs[ENTITY.ccols.index(F["alchemy_level"])] == 100  # as the reference has them
    assert ENTITY.cdivs[ENTITY.ccols.index(F["alchemy_exp"])] == 10
    assert (ITEM.cols, ITEM.D, ITEM.C, ITEM.features, ITEM.bias) == (16, 2, 12, 76, 524)
    assert ITEM.dcols == (1, 14) and ITEM.doffs == (2, 0)
    assert ITEM.ccols == (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15)
    assert ITEM.cdivs == (10, 10, 10, 100, 100, 100, 40, 40, 40, 100, 100, 100)


def test_header_symbols_and_ctypes_agree():
    text = open(os.path.join(ROOT, "include", "nmmo_heads.h")).read()
    L = heads.lib()
    for sym in NEW:
        assert sym in heads.SYMBOLS
        (params,) = re.findall(rf"NMH_API\s+int\s+{sym}\s*\(([^)]*)\)", text)
        assert len(getattr(L, sym).argtypes) == len(params.split(",")), sym
    # the kind first, then the item calls' arguments
    assert L.nmh_embed_logits.argtypes[1:] == L.nmh_item_logits.argtypes
    assert L.nmh_embed_logits_backward.argtypes[1:] == L.nmh_item_logits_backward.argtypes


class Args:
    """Valid arguments with no rows; a test bends one of them."""

    def __init__(self, kind=ENTITY, set_rows=12, n_heads=3):
        self.code, self.n = kind.code, 0
        self.set, self.set_stride, self.elem, self.set_rows, self.share = DUMMY, kind.cols * set_rows, 0, set_rows, 1
        self.ids, self.id_stride, self.id_kind = DUMMY, 1, 0
        own = DUMMY if kind is ENTITY else None
        self.outs = dict(idx=DUMMY, cont=DUMMY, counts=DUMMY, sums=DUMMY, mine_idx=own, mine_i=own, mine_c=own)
        self.mask = self.pq = self.out = self.g_out = self.g_pq = DUMMY
        self.mask_kind = heads.MASK_F32
        width = set_rows + 1
        self.sh = ctypes.byref(_sets.set_heads_struct([7 + h * width for h in range(n_heads)],
                                                      [h * width for h in range(n_heads)], kind.name))
        self.mask_stride, self.out_stride = 7 + n_heads * width, n_heads * width

    def features(self):
        return heads.lib().nmh_embed_features(self.code, self.n, self.set, self.set_stride, self.elem, self.set_rows,
                                              self.ids, self.id_stride, self.id_kind, *self.outs.values(), None)

    def logits(self):
        return heads.lib().nmh_embed_logits(self.code, self.sh, self.n, self.set, self.set_stride, self.elem,
                                            self.set_rows, self.share, self.mask, self.mask_stride, self.mask_kind,
                                            self.pq, self.out, self.out_stride, None)

    def logits_backward(self):
        return heads.lib().nmh_embed_logits_backward(
            self.code, self.sh, self.n, self.set, self.set_stride, self.elem, self.set_rows, self.share, self.mask,
            self.mask_stride, self.mask_kind, self.g_out, self.out_stride, self.g_pq, None)


FNS = ["features", "logits", "logits_backward"]


def refused(a, fn, *words):
    rc = getattr(a, fn)()
    msg = heads.lib().nmh_last_error().decode()
    assert rc == heads.NMH_E_INVALID, (fn, rc, msg)
    assert msg.startswith(f"nmh_embed_{fn}:"), msg
    for w in words:
        assert w in msg, (fn, w, msg)
    return msg


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k.name)
def test_valid_arguments_with_no_rows_are_a_no_op(kind):
    for a in (Args(kind), Args(kind, 1, 1), Args(kind, kind.max_rows, 1)):
        assert a.features() == a.logits() == a.logits_backward() == heads.NMH_OK
        a.elem, a.id_kind, a.mask_kind, a.share = 1, 1, heads.MASK_U8, 3
        a.set_stride = a.id_stride = 23987
        assert a.features() == a.logits() == a.logits_backward() == heads.NMH_OK
        for keep in [k for k, v in a.outs.items() if v]:  # any output alone
            outs = dict(a.outs)
            a.outs = {k: DUMMY if k == keep else None for k in outs}
            assert a.features() == heads.NMH_OK, keep
            a.outs = outs
        a.outs.update(mine_idx=None, mine_i=None, mine_c=None)  # no own row: no ids, and nothing about them is looked at
        a.ids, a.id_kind, a.id_stride = None, 9, 0
        assert a.features() == heads.NMH_OK


@pytest.mark.parametrize("fn", FNS)
def test_a_bad_kind_is_refused_first(fn):
    for code in (2, -1):
        a = Args()
        a.code, a.set = code, None
        assert refused(a, fn, "kind", str(code)) == f"nmh_embed_{fn}: unknown kind {code}"


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k.name)
@pytest.mark.parametrize("fn", FNS)
def test_bad_element_kind_rows_stride_and_pointers_are_refused(fn, kind):
    for elem in (2, -1):
        a = Args(kind)
        a.elem = elem
        refused(a, fn, "elem_kind", str(elem))
    for rows in (0, kind.max_rows + 1, -1):
        a = Args(kind)
        a.set_rows, a.set_stride, a.mask_stride, a.out_stride = rows, 1 << 20, 1 << 20, 1 << 20
        assert refused(a, fn, "set_rows").endswith(f"set_rows {rows} outside 1..{kind.max_rows}")
    a = Args(kind, 100 if kind is ENTITY else 12)
    a.set_stride -= 1
    refused(a, fn, "set_stride", str(a.set_stride))
    a = Args(kind)
    a.set = None
    assert refused(a, fn).endswith("set is NULL")
    a = Args(kind)
    a.n = -1
    refused(a, fn, "n_sets" if fn == "features" else "n_rows", "-1")


def test_features_without_an_output_without_ids_or_of_the_wrong_kind_are_refused():
    a = Args()
    a.outs = {k: None for k in a.outs}
    refused(a, "features", "every output is NULL")
    for keep in ("mine_idx", "mine_i", "mine_c"):
        a = Args()
        a.outs = {k: DUMMY if k == keep else None for k in a.outs}
        a.ids = None
        refused(a, "features", "ids", "NULL")
        b = Args(ITEM)
        b.outs[keep] = DUMMY
        refused(b, "features", "entity kind")
    for id_kind in (2, -1):
        a = Args()
        a.id_kind = id_kind
        refused(a, "features", "id_kind", str(id_kind))
    for stride in (0, -5):
        a = Args()
        a.id_stride = stride
        refused(a, "features", "id_stride", str(stride))


@pytest.mark.parametrize("fn", ["logits", "logits_backward"])
def test_bad_heads_strides_and_pointers_are_refused(fn):
    for n_heads in (0, 5, -1):
        a = Args()
        sh = _sets.set_heads_struct([0], [0], "entity")
        sh.n_heads = n_heads
        a.sh = ctypes.byref(sh)
        assert refused(a, fn).endswith(f"n_heads {n_heads} outside 1..4")
    a = Args()
    a.sh = None
    assert refused(a, fn).endswith("sh is NULL")
    a = Args()
    a.share = 0
    refused(a, fn, "share", "0")
    for field, word in (("mask_stride", "mask_stride"), ("out_stride", "out_stride" if fn == "logits" else "g_stride")):
        a = Args()
        setattr(a, field, getattr(a, field) - 1)
        refused(a, fn, word)
    for field in ("mask",) + (("pq", "out") if fn == "logits" else ("g_out", "g_pq")):
        a = Args()
        setattr(a, field, None)
        assert refused(a, fn).endswith(f"{field} is NULL")
    a = Args()
    a.mask_kind = 2
    refused(a, fn, "mask_kind", "2")
    if fn == "logits":
        a = Args()
        a.pq = DUMMY + 4
        refused(a, fn, "pq", "16-byte aligned")


def test_the_python_wrappers_refuse_host_tensors_and_bad_shapes():
    x = torch.zeros((2, 4, 31))
    with pytest.raises(heads.HeadsError, match="run on the GPU"):
        embed.embed_features(ENTITY, x)
    with pytest.raises(heads.HeadsError, match="runs on the GPU"):
        embed.embed_logits(ENTITY, x, torch.zeros((2, 1, ENTITY.query)), torch.zeros((2, 5)), [0])
    for enc in (embed.ReducedPlayerEncoder(8, 8, fused=True), embed.ReducedItemEncoder(8, 8, fused=True)):
        with pytest.raises(heads.HeadsError):
            enc.pooled(torch.zeros((2, 4, enc.kind.cols)))
    with pytest.raises(ValueError, match="between 1 and 4 heads"):
        _sets.set_heads_struct(range(5), range(5), "entity")
    # item_logits and player_logits keep their specs: no kind argument
    assert item.SPEC.kind is None and player.SPEC.kind is None
    assert ENTITY.spec.kind == 0 and ITEM.spec.kind == 1 and ENTITY.spec.query == 1052 and ITEM.spec.query == 528


# ---------------------------------------------------------------- the rule in plain torch
ENTITY_EDGES = {0: [-32767, -1, 0, 1, 128, 255, 256, 32767, -0.5, 0.99, 254.5, 255.5],
                1: [-257, -256, -255, -1, 0, -255.5], 8: [-513, -512, -511, -258, -257, -256],
                10: [-769, -768, -767, -514, -513, -512]}
ITEM_EDGES = {1: [-3, -2, -1, 0, 17, 253, 254, -2.5, 252.99], 14: [-1, 0, 1, 255, 256]}


def numpy_features(kind, x):
    """SPEC §25 in numpy: idx = clip(trunc(x + off), 0, 255), NaN -> 0; cont = x / s in x's dtype."""
    v = x[..., list(kind.dcols)] + np.asarray(kind.doffs, dtype=x.dtype)
    idx = np.clip(np.trunc(np.where(np.isnan(v), 0, v)), 0, 255).astype(np.int64)
    return idx, x[..., list(kind.ccols)] / np.asarray(kind.cdivs, dtype=x.dtype)


@pytest.mark.parametrize("kind,edges", [(ENTITY, ENTITY_EDGES), (ITEM, ITEM_EDGES)], ids=["entity", "item"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int16])
def test_embed_features_ref_equals_numpy_bit_for_bit_on_the_edges(kind, edges, dtype):
    rng = np.random.default_rng(0)
    x = rng.integers(-300, 3000, (3, 40, kind.cols)).astype(np.float64)
    x[0, :, list(kind.ccols)[-1]] = 32767
    x[1, :, list(kind.ccols)[0]] = -32767
    for col, vals in edges.items():
        x[0, :len(vals), col] = vals
        if dtype is not np.int16:
            x[1, 0, col] = np.nan
    x = np.trunc(x).astype(dtype) if dtype is np.int16 else x.astype(dtype)
    idx, cont = embed.embed_features_ref(kind, torch.from_numpy(x))
    f = x.astype(np.float32) if dtype is np.int16 else x
    want_idx, want_cont = numpy_features(kind, f)
    assert idx.dtype == torch.int64 and np.array_equal(idx.numpy(), want_idx)
    assert cont.numpy().dtype == f.dtype and cont.numpy().tobytes() == want_cont.tobytes()
    assert idx.min() == 0 and idx.max() == 255
    if kind is ENTITY:  # the offset columns saturate: every value >= -1 (-257, -513) reads bin 255
        plain = torch.from_numpy(np.abs(f[2]))
        assert bool((embed.embed_features_ref(kind, plain)[0][:, 1:] == 255).all())


@pytest.mark.parametrize("cls", [embed.ReducedPlayerEncoder, embed.ReducedItemEncoder])
def test_pointer_query_and_the_pool_reproduce_the_materialised_chain_in_float64(cls):
    torch.manual_seed(1)
    enc = cls(24, 40).double().requires_grad_(False)
    k, n, R, H = enc.kind, 3, 17, 4
    x = torch.randint(-300, 300, (n, R, k.cols)).double()
    for d, col in enumerate(k.dcols):
        x[:, :, col] = torch.randint(-5, 260, (n, R)).double() - k.doffs[d] * torch.randint(0, 2, (n, R))
    q = torch.randn(n, H, 40).double()
    emb = enc.embed(x)  # [n, R, 40]
    want = torch.einsum("nhk,njk->nhj", q, emb)
    pq = enc.pointer_query(q)
    assert pq.shape == (n, H, k.query) and not bool(pq[..., k.bias + 1:].any())
    idx, cont = embed.embed_features_ref(k, x)
    got = pq[..., k.bias].unsqueeze(-1).expand(n, H, R).clone()  # SPEC §25's order
    for d in range(k.D):
        got += torch.gather(pq[..., d * 256:(d + 1) * 256], 2, idx[..., d].unsqueeze(1).expand(n, H, R))
    for c in range(k.C):
        got += cont[..., c].unsqueeze(1) * pq[..., k.D * 256 + c].unsqueeze(-1)
    scale = float(torch.einsum("nhk,njk->nhj", q.abs(), emb.abs()).max())
    assert float((got - want).abs().max()) <= 1e-12 * max(scale, 1.0)
    # the pool: counts and sums as the kernel returns them
    counts = torch.nn.functional.one_hot(idx, 256).sum(1).double()
    sums = x[..., list(k.ccols)].sum(1)
    mean_e = (counts @ enc.embedding.weight[:256]).flatten(-2) / R
    mean_c = sums / torch.tensor(k.cdivs, dtype=torch.float64) / R
    pooled = enc._fc(torch.cat([mean_e, mean_c], -1))
    assert float((pooled - emb.mean(1)).abs().max()) <= 1e-12 * max(float(emb.abs().max()), 1.0)
