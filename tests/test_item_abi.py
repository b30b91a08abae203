"""The item-encoder entry points of libnmmo_heads.so (include/nmmo_heads.h, SPEC.md §20) and
nmmo_amd/item.py without a GPU: the constants match the header as a C compiler reads it, every
argument rule is refused with NMH_E_INVALID and a message naming the field (every call passes dummy
non-null pointers and n_rows = 0, so a missing check shows as NMH_OK, never as a launch),
`item_features_ref` is the reference's lines 162-168, and in float64 the pooled embedding and the
projected-query logits equal the materialised chain (embed, pad, matmul, mean). CPU only."""

import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from nmmo_amd import heads, item

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = 0x1000  # non-null, 16-byte aligned, never dereferenced


def test_constants_match_the_c_compiler():
    src = r"""
#include <stdio.h>
#include <stddef.h>
#include "nmmo_heads.h"
int main(void) {
  printf("%d %d %d %d %d %d %d %d %d %d %d\n", NMH_ITEM_COLS, NMH_ITEM_FEATURES, NMH_ITEM_TYPES, NMH_ITEM_QUERY,
         NMH_ITEM_MAX_ROWS, NMH_ITEM_MAX_HEADS, NMH_ITEM_F32, NMH_ITEM_I16, (int)sizeof(NmhItemHeads),
         (int)offsetof(NmhItemHeads, mask_off), (int)offsetof(NmhItemHeads, out_off));
  return 0;
}
"""
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        with open(c, "w") as fh:
            fh.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [item.COLS, item.FEATURES, item.TYPES, item.QUERY, item.MAX_ROWS, item.MAX_HEADS, item.ITEM_F32,
                   item.ITEM_I16, ctypes.sizeof(item.NmhItemHeads), item.NmhItemHeads.mask_off.offset,
                   item.NmhItemHeads.out_off.offset]
    assert got == [16, 32, 18, 36, 1024, 4, 0, 1, 36, 4, 20]
    assert item.CONT_COLS == [3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15] and (item.TYPE_COL, item.EQUIPPED_COL) == (1, 14)


class Args:
    """Valid arguments with no rows; a test bends one of them."""

    def __init__(self, set_rows=12, n_heads=4):
        self.n = 0
        self.items, self.item_stride, self.kind, self.set_rows, self.share = DUMMY, 16 * set_rows, item.ITEM_F32, set_rows, 1
        self.features = self.sums = self.mask = self.pq = self.out = self.g_out = self.g_pq = DUMMY
        self.mask_kind = heads.MASK_F32
        width = set_rows + 1
        self.ih = item.item_heads_struct([7 + h * width for h in range(n_heads)], [h * width for h in range(n_heads)])
        self.mask_stride, self.out_stride = 7 + n_heads * width, n_heads * width

    def features_(self):
        return heads.lib().nmh_item_features(self.n, self.items, self.item_stride, self.kind, self.set_rows,
                                             self.features, self.sums, None)

    def logits(self):
        return heads.lib().nmh_item_logits(ctypes.byref(self.ih), self.n, self.items, self.item_stride, self.kind,
                                           self.set_rows, self.share, self.mask, self.mask_stride, self.mask_kind,
                                           self.pq, self.out, self.out_stride, None)

    def logits_backward(self):
        return heads.lib().nmh_item_logits_backward(
            ctypes.byref(self.ih), self.n, self.items, self.item_stride, self.kind, self.set_rows, self.share,
            self.mask, self.mask_stride, self.mask_kind, self.g_out, self.out_stride, self.g_pq, None)


FNS = {"features": "features_", "logits": "logits", "logits_backward": "logits_backward"}


def refused(a, fn, *words):
    rc = getattr(a, FNS[fn])()
    msg = heads.lib().nmh_last_error().decode()
    assert rc == heads.NMH_E_INVALID, (fn, rc, msg)
    assert msg.startswith(f"nmh_item_{fn}:"), msg
    for w in words:
        assert w in msg, (fn, w, msg)


def test_valid_arguments_with_no_rows_are_a_no_op():
    for a in (Args(), Args(1, 1), Args(1024, 1), Args(1024, 4)):
        assert a.features_() == a.logits() == a.logits_backward() == heads.NMH_OK
        a.kind, a.mask_kind, a.share, a.item_stride = item.ITEM_I16, heads.MASK_U8, 128, 23987 + 16 * 1024
        assert a.features_() == a.logits() == a.logits_backward() == heads.NMH_OK
        a.features = None  # either output alone
        assert a.features_() == heads.NMH_OK
        a.features, a.sums = DUMMY, None
        assert a.features_() == heads.NMH_OK


@pytest.mark.parametrize("fn", sorted(FNS))
def test_bad_kind_rows_and_stride_are_refused(fn):
    for kind in (2, -1):
        a = Args()
        a.kind = kind
        refused(a, fn, "item_kind", str(kind))
    for rows in (0, 1025, -1):
        a = Args()
        a.set_rows, a.item_stride, a.mask_stride, a.out_stride = rows, 1 << 20, 1 << 20, 1 << 20
        refused(a, fn, "set_rows", str(rows))
    a = Args(12)
    a.item_stride = 16 * 12 - 1
    refused(a, fn, "item_stride", "191")
    a = Args()
    a.items = None
    refused(a, fn, "items", "NULL")
    a = Args()
    a.n = -1
    refused(a, fn, "n_sets" if fn == "features" else "n_rows", "-1")


def test_features_without_an_output_are_refused():
    a = Args()
    a.features = a.sums = None
    refused(a, "features", "features", "sums", "NULL")


@pytest.mark.parametrize("fn", ["logits", "logits_backward"])
def test_bad_share_heads_strides_and_pointers_are_refused(fn):
    for share in (0, -2):
        a = Args()
        a.share = share
        refused(a, fn, "share", str(share))
    for n_heads in (0, 5, -1):
        a = Args()
        a.ih.n_heads = n_heads
        refused(a, fn, "n_heads", str(n_heads))
    a = Args(12, 4)  # the furthest head ends at 3 * 13 + 13 = 52
    a.out_stride = 51
    refused(a, fn, "out_stride" if fn == "logits" else "g_stride", "51")
    a.out_stride = 52
    assert getattr(a, fn)() == heads.NMH_OK
    a.ih.out_off[1] = 40  # heads need not be in order: the furthest counts
    refused(a, fn, "out_stride" if fn == "logits" else "g_stride", "52")
    a = Args(12, 4)
    a.mask_stride -= 1
    refused(a, fn, "mask_stride", str(a.mask_stride))
    a = Args()
    a.ih.mask_off[2] = -1
    refused(a, fn, "mask_off")
    a = Args()
    a.mask_kind = 2
    refused(a, fn, "mask_kind", "2")
    for field in ("mask", "pq", "out") if fn == "logits" else ("mask", "g_out", "g_pq"):
        a = Args()
        setattr(a, field, None)
        refused(a, fn, field, "NULL")
    rc = getattr(heads.lib(), f"nmh_item_{fn}")(None, 0, DUMMY, 192, 0, 12, 1, DUMMY, 99, 0, DUMMY, *(
        (DUMMY, 99, None) if fn == "logits" else (99, DUMMY, None)))
    assert rc == heads.NMH_E_INVALID and b"ih is NULL" in heads.lib().nmh_last_error()


def test_misaligned_pq_is_refused():
    a = Args()
    a.pq = DUMMY + 4
    refused(a, "logits", "pq", "16-byte")
    a = Args()
    a.out = a.items = a.mask = DUMMY + 4  # nothing else needs more than its element's alignment
    a.g_out = a.g_pq = DUMMY + 4
    assert a.logits() == heads.NMH_OK and a.logits_backward() == heads.NMH_OK


# ---------------------------------------------------------------- nmmo_amd/item.py
def reference_features(items):
    """baseline_policy.py:162-168, literally (one_hot raises outside the classes)."""
    discrete_idxs, continuous_idxs = [1, 14], [3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15]
    assert discrete_idxs == [item.TYPE_COL, item.EQUIPPED_COL]
    continuous_scale = torch.Tensor([1 / 100] * 12)
    one_hot_discrete_equipped = F.one_hot(items[:, :, 14].long(), num_classes=2).float()
    one_hot_discrete_type_id = F.one_hot(items[:, :, 1].long(), num_classes=18).float()
    one_hot_discrete = torch.concat([one_hot_discrete_type_id, one_hot_discrete_equipped], dim=-1)
    continuous = items[:, :, continuous_idxs] * continuous_scale
    return torch.cat([one_hot_discrete, continuous], dim=-1).float()


def sample_items(m, rows, rng, in_range=True):
    """[m, rows, 16] float32 item sets with integer values: mostly empty slots, every type."""
    x = rng.integers(-200, 2000, (m, rows, 16)).astype(np.float32)
    x[:, :, 1] = rng.integers(0, 18, (m, rows))
    x[:, :, 14] = rng.integers(0, 2, (m, rows))
    x[rng.random((m, rows)) < 0.5] = 0
    if not in_range:
        x[0, 0, 1], x[0, 0, 14] = -3, 5
        x[0, -1, 1], x[0, -1, 14] = 40, -1
        x[-1, 0, 1] = np.nan
        x[-1, 0, 14] = np.nan
    return torch.from_numpy(x)


def test_item_features_ref_is_the_references_lines_where_those_are_defined():
    x = sample_items(5, 12, np.random.default_rng(0))
    got = item.item_features_ref(x)
    assert got.dtype == torch.float32 and got.shape == (5, 12, 32)
    assert torch.equal(got, reference_features(x))
    assert torch.equal(item.item_features_ref(x.to(torch.int16)), got)
    assert torch.equal(item.item_features_ref(x.reshape(60, 16)), got.reshape(60, 32))
    d = item.item_features_ref(x.double())
    assert d.dtype == torch.float64 and torch.equal(d[..., :20], got[..., :20].double())
    assert torch.equal(d[..., 20:], x[..., item.CONT_COLS].double() * float(np.float32(0.01)))


def test_item_features_ref_clamps_where_one_hot_would_raise():
    x = sample_items(3, 4, np.random.default_rng(1), in_range=False)
    with pytest.raises(RuntimeError):
        reference_features(x)
    f = item.item_features_ref(x)
    assert f[0, 0, :18].argmax() == 0 and f[0, 0, 18:20].argmax() == 1  # type -3 -> 0, equipped 5 -> 1
    assert f[0, -1, :18].argmax() == 17 and f[0, -1, 18:20].argmax() == 0  # type 40 -> 17, equipped -1 -> 0
    assert f[-1, 0, 0] == 1 and f[-1, 0, 18] == 1  # NaN -> class 0
    assert torch.equal(f[..., :18].sum(-1), torch.ones(3, 4)) and torch.equal(f[..., 18:20].sum(-1), torch.ones(3, 4))


@torch.no_grad()
def test_pooled_and_projected_query_logits_equal_the_materialised_chain_in_float64():
    torch.manual_seed(0)
    rng = np.random.default_rng(2)
    enc = item.ItemEncoder(24).double()
    market_fc = torch.nn.Linear(24, 24).double()
    for rows in (1, 12, 65):
        x = sample_items(4, rows, rng).double()
        q = torch.randn(4, 3, 24, dtype=torch.float64)
        emb = enc.embed(x)  # the reference's chain: embed, pad, matmul, mean
        padded = torch.cat([emb, emb.new_zeros(4, 1, 24)], 1)
        want = torch.stack([torch.matmul(padded, q[:, h].unsqueeze(-1)).squeeze(-1) for h in range(3)], 1)
        want_market = market_fc(emb).mean(-2)
        # what the fused path computes: sums / R through fc, and pq . (x, 1)
        feats = item.item_features_ref(x)
        pooled = F.linear(feats.sum(1) / rows, enc.fc.weight, enc.fc.bias)
        pq = enc.pointer_query(q)
        assert pq.shape == (4, 3, 36) and torch.equal(pq[..., 33:], torch.zeros(4, 3, 3, dtype=torch.float64))
        got = torch.einsum("nhf,njf->nhj", pq[..., :32], feats) + pq[..., 32:33]
        scale = max(1.0, float(want.abs().max()))
        assert float((got - want[..., :rows]).abs().max()) <= 1e-12 * scale
        assert torch.equal(want[..., rows], torch.zeros(4, 3, dtype=torch.float64))  # the no-op: the zero row
        assert float((pooled - enc.pooled(x)).abs().max()) <= 1e-12 * max(1.0, float(pooled.abs().max()))
        assert float((market_fc(pooled) - want_market).abs().max()) <= 1e-12 * max(1.0, float(want_market.abs().max()))


def test_item_encoder_parameter_names_are_the_references():
    for fused in (False, True):
        sd = item.ItemEncoder(256, fused=fused).state_dict()
        assert {k: tuple(v.shape) for k, v in sd.items()} == {"fc.weight": (256, 32), "fc.bias": (256,)}
    a, b = item.ItemEncoder(32), item.ItemEncoder(32, fused=True)
    b.load_state_dict(a.state_dict())
    a.load_state_dict(b.state_dict())


def test_host_tensors_are_refused_without_a_fallback():
    enc = item.ItemEncoder(32, fused=True)
    x = torch.zeros((2, 12, 16))
    for call in (lambda: item.item_features(x), lambda: item.item_sums(x), lambda: enc.embed(x), lambda: enc.pooled(x),
                 lambda: item.item_logits(x, torch.zeros(2, 1, 36), torch.ones(2, 13), [0])):
        with pytest.raises(heads.HeadsError, match="GPU"):
            call()


def test_item_agent_defaults_to_unfused_and_keeps_the_stand_ins_call_convention():
    from nmmo_amd import layout
    from nmmo_amd.trainer import ItemMaskedAgent

    torch.manual_seed(0)
    agent = ItemMaskedAgent(16, hidden=32)
    assert not agent.item_encoder.fused and not agent.fused_heads
    assert ItemMaskedAgent(16, hidden=32, fused_item=True).item_encoder.fused
    assert sum(agent.dims) == 1586 and len(agent.queries) == 5 and len(agent.dense) == 7
    obs = torch.zeros((3, layout.obs_elems(16)))
    obs[:, :sum(agent.dims)] = 1.0
    keep = obs.clone()
    a, logp, ent, value = agent(obs)
    assert torch.equal(obs, keep)
    assert a.shape == (3, len(agent.dims)) and logp.shape == ent.shape == (3,) and value.shape == (3, 1)
    _, logp2, _, _ = agent(obs, action=a)
    assert torch.allclose(logp, logp2)
    assert {n.split(".")[0] for n, _ in agent.named_parameters()} == {
        "encoder", "item_encoder", "inventory", "market", "queries", "dense", "value"}
    assert {k for k in agent.state_dict() if k.startswith("item_encoder.")} == {"item_encoder.fc.weight",
                                                                                "item_encoder.fc.bias"}
