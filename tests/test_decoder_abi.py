"""nmh_decoder_forward / nmh_decoder_backward of libnmmo_heads.so (include/nmmo_heads.h, SPEC.md §23)
and `decoder.decoder_heads` without a GPU: the new constants and the struct's layout match the header
as a C compiler reads it, every argument rule is refused with NMH_E_INVALID and a message naming the
field (every call passes dummy non-null pointers and n_rows = 0, so a missing check shows as NMH_OK,
never as a launch), and `spec_decoder_tile`, the numpy restatement of §23's staged tile that the GPU
tests lean on, is what it says it is. CPU only.

`spec_decoder_tile` adds term by term in §20's and §21's order with one rounding per fused
multiply-add. Torch's composed expressions (`item_features_ref` / `player_features_ref`,
`pointer_query`, a product and a sum, a masked fill of 0 / -inf) add in another order, so the two are
compared twice: for equality on inputs where every partial sum is exact in any order (integer columns,
integer weights, and zero weights on the items' scaled columns, whose features col * 0.01f have full
mantissas), and on general float weights, scaled columns included, against the float64 chain within
the roundings of the chain."""

import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from nmmo_amd import decoder, heads, item, player
from tests.test_gpu_item import make_sets as make_item_sets
from tests.test_gpu_player import make_sets as make_entity_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = 0x1000  # non-null, 16-byte aligned, never dereferenced
F32 = np.float32
EPS = 2.0 ** -24


# ---------------------------------------------------------------- constants
def test_new_constants_and_the_struct_match_the_c_compiler():
    src = r"""
#include <stdio.h>
#include <stddef.h>
#include "nmmo_heads.h"
int main(void) {
  printf("%d %d %d %d %d %d %d %d %d %d %d %d %d\n", NMH_SET_ENTITY, NMH_SET_ITEM, NMH_ELEM_F32, NMH_ELEM_I16,
         NMH_DECODER_QUERY, NMH_MAX_SETS, NMH_MAX_HEADS, (int)sizeof(NmhDecoderSets),
         (int)offsetof(NmhDecoderSets, rule), (int)offsetof(NmhDecoderSets, share),
         (int)offsetof(NmhDecoderSets, head_set), (int)offsetof(NmhDecoderSets, stride),
         (int)offsetof(NmhDecoderSets, base));
  return 0;
}
"""
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        with open(c, "w") as fh:
            fh.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    S = decoder.NmhDecoderSets
    assert got == [decoder.SET_ENTITY, decoder.SET_ITEM, decoder.ELEM_F32, decoder.ELEM_I16, decoder.QUERY,
                   heads.MAX_SETS, heads.MAX_HEADS, ctypes.sizeof(S), S.rule.offset, S.share.offset,
                   S.head_set.offset, S.stride.offset, S.base.offset]
    assert got == [0, 1, 0, 1, 40, 4, 16, 184, 8, 40, 56, 120, 152]
    assert decoder.QUERY >= player.QUERY >= item.QUERY
    assert (decoder.ELEM_F32, decoder.ELEM_I16) == (item.ITEM_F32, item.ITEM_I16) == (player.PLAYER_F32, player.PLAYER_I16)


# ---------------------------------------------------------------- argument rules
class Args:
    """Valid arguments with no rows: a dense head of 3, an entity head over 5 candidates, two item
    heads over 8 and a dense head of 7. A test bends one of them."""

    def __init__(self):
        self.dims = [3, 6, 9, 9, 7]
        self.head_set = [-1, 0, 1, 1, -1]
        self.rules, self.rows, self.shares = [decoder.SET_ENTITY, decoder.SET_ITEM], [5, 8], [1, 1]
        self.strides, self.bases, self.elem = [31 * 5, 16 * 8], [DUMMY, DUMMY], decoder.ELEM_F32
        self.n = 0
        self.pq = self.dense = self.mask = self.actions = self.a_out = self.logprob = self.entropy = DUMMY
        self.lse = self.hent = self.g_logprob = self.g_entropy = self.g_dense = self.g_pq = DUMMY
        self.dense_stride, self.mask_stride, self.mask_kind, self.g_dense_stride = 10, 34, heads.MASK_F32, 10
        self.hd = self.st = True  # False: pass NULL

    def structs(self):
        hd = heads.NmhHeads()
        hd.n_heads = len(self.dims)
        for k, d in enumerate(self.dims[:heads.MAX_HEADS]):
            hd.dims[k] = d
        st = decoder.NmhDecoderSets()
        st.n_sets, st.elem_kind = len(self.rules), self.elem
        for s in range(min(len(self.rules), heads.MAX_SETS)):
            st.rule[s], st.set_rows[s], st.share[s] = self.rules[s], self.rows[s], self.shares[s]
            st.stride[s], st.base[s] = self.strides[s], self.bases[s]
        for k, s in enumerate(self.head_set[:heads.MAX_HEADS]):
            st.head_set[k] = s
        return (ctypes.byref(hd) if self.hd else None), (ctypes.byref(st) if self.st else None)

    def forward(self):
        hd, st = self.structs()
        return heads.lib().nmh_decoder_forward(hd, st, self.n, self.pq, self.dense, self.dense_stride, self.mask,
                                               self.mask_stride, self.mask_kind, self.actions, 1, 2, 3, self.a_out,
                                               self.logprob, self.entropy, self.lse, self.hent, None)

    def backward(self):
        hd, st = self.structs()
        return heads.lib().nmh_decoder_backward(hd, st, self.n, self.pq, self.dense, self.dense_stride, self.mask,
                                                self.mask_stride, self.mask_kind, self.actions, self.lse, self.hent,
                                                self.g_logprob, self.g_entropy, self.g_dense, self.g_dense_stride,
                                                self.g_pq, None)


FNS = ["forward", "backward"]


def refused(a, fn, *words):
    rc = getattr(a, fn)()
    msg = heads.lib().nmh_last_error().decode()
    assert rc == heads.NMH_E_INVALID, (fn, rc, msg)
    assert msg.startswith(f"nmh_decoder_{fn}:"), msg
    for w in words:
        assert str(w) in msg, (fn, w, msg)


def bent(**kw):
    a = Args()
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_valid_arguments_with_no_rows_are_a_no_op():
    a = Args()
    assert a.forward() == a.backward() == heads.NMH_OK
    a = bent(elem=decoder.ELEM_I16, mask_kind=heads.MASK_U8, shares=[1, 128], strides=[23987, 16 * 1024], actions=None)
    assert a.forward() == heads.NMH_OK  # sampling
    a = bent(g_logprob=None, g_entropy=None)
    assert a.backward() == heads.NMH_OK
    assert bent(g_dense=None).backward() == bent(g_pq=None).backward() == bent(g_dense=None, g_pq=None).backward() == 0
    # every head dense: no sets, no pq
    a = bent(dims=[3, 7], head_set=[-1, -1], rules=[], rows=[], shares=[], strides=[], bases=[], pq=None)
    assert a.forward() == a.backward() == heads.NMH_OK
    # every head a pointer head: no dense
    a = bent(dims=[6, 9], head_set=[0, 1], dense=None, g_dense=None)
    assert a.forward() == a.backward() == heads.NMH_OK
    # the nmmo heads, and the largest sets
    nmmo = dict(dims=[3, 101, 1025, 13, 13, 101, 99, 101, 5, 13, 99, 13], head_set=[-1, 0, 2, 1, 1, 0, -1, 0, -1, 1, -1, 1],
                rules=[0, 1, 1], rows=[100, 12, 1024], shares=[1, 1, 1], strides=[23987] * 3, bases=[DUMMY] * 3,
                dense_stride=206, g_dense_stride=206, mask_stride=23987)
    assert bent(**nmmo).forward() == bent(**nmmo).backward() == heads.NMH_OK
    a = bent(dims=[257, 1025], head_set=[0, 1], rows=[256, 1024], strides=[31 * 256, 16 * 1024], mask_stride=1282)
    assert a.forward() == a.backward() == heads.NMH_OK


@pytest.mark.parametrize("fn", FNS)
def test_bad_counts_and_kinds_are_refused(fn):
    refused(bent(hd=False), fn, "hd", "NULL")
    refused(bent(st=False), fn, "sets", "NULL")
    refused(bent(dims=[]), fn, "n_heads", 0)
    refused(bent(dims=[1] * 17, head_set=[-1] * 17), fn, "n_heads", 17)
    refused(bent(rules=[0, 1, 1, 1, 1], rows=[5, 8, 8, 8, 8], shares=[1] * 5, strides=[999] * 5, bases=[DUMMY] * 5), fn,
            "n_sets", 5)
    for kind in (2, -1):
        refused(bent(elem=kind), fn, "elem_kind", kind)
        refused(bent(mask_kind=kind), fn, "mask_kind", kind)
        refused(bent(rules=[kind, 1]), fn, "rule[0]", kind)
    refused(bent(n=-1), fn, "n_rows", -1)


@pytest.mark.parametrize("fn", FNS)
def test_bad_sets_are_refused(fn):
    big = dict(strides=[1 << 20, 1 << 20], mask_stride=1 << 20)
    for rows in (0, -1, 257):  # an entity set has 1..256 candidates
        refused(bent(rows=[rows, 8], dims=[3, rows + 1, 9, 9, 7], **big), fn, "set_rows[0]", rows)
    for rows in (0, 1025):  # an item set 1..1024
        refused(bent(rows=[5, rows], dims=[3, 6, rows + 1, rows + 1, 7], **big), fn, "set_rows[1]", rows)
    refused(bent(strides=[31 * 5 - 1, 16 * 8]), fn, "stride[0]", 154)
    refused(bent(strides=[31 * 5, 16 * 8 - 1]), fn, "stride[1]", 127)
    for share in (0, -3):
        refused(bent(shares=[1, share]), fn, "share[1]", share)
    refused(bent(bases=[DUMMY, None]), fn, "base[1]", "NULL")
    refused(bent(dims=[3, 7, 9, 9, 7], mask_stride=35), fn, "dims[1]", "set_rows[0] + 1")  # dims[k] != R + 1
    refused(bent(dims=[3, 6, 9, 8, 7]), fn, "dims[3]", "set_rows[1] + 1")
    refused(bent(head_set=[-1, 0, 0, 0, -1], dims=[3, 6, 6, 6, 7]), fn, "no head uses set 1")  # an unused set
    refused(bent(head_set=[-1, 2, 1, 1, -1]), fn, "head_set[1]", 2)
    refused(bent(head_set=[-2, 0, 1, 1, -1]), fn, "head_set[0]", -2)
    refused(bent(dims=[0, 6, 9, 9, 7]), fn, "dims[0]", 0)


@pytest.mark.parametrize("fn", FNS)
def test_bad_strides_pointers_and_totals_are_refused(fn):
    refused(bent(mask_stride=33), fn, "mask_stride", 33, 34)
    refused(bent(dense_stride=9), fn, "dense_stride", 9, 10)
    # sum(dims) > NMH_MAX_DIM with every head within its own limits
    refused(bent(dims=[1025, 1025], head_set=[0, 0], rules=[1], rows=[1024], shares=[1], strides=[16384], bases=[DUMMY],
                 mask_stride=1 << 20, dense=None), fn, "sum(dims)", 2050, 2048)
    refused(bent(mask=None), fn, "mask", "NULL")
    refused(bent(dense=None), fn, "dense", "NULL")
    refused(bent(pq=None), fn, "pq", "NULL")
    refused(bent(pq=DUMMY + 4), fn, "pq", "16-byte")


def test_each_null_output_and_backward_rule_is_refused():
    for name in ("a_out", "logprob", "entropy", "lse", "hent"):
        refused(bent(**{name: None}), "forward", "output", "NULL")
    for name in ("actions", "lse", "hent"):
        refused(bent(**{name: None}), "backward", "actions, lse or head_entropy", "NULL")
    refused(bent(g_dense_stride=9), "backward", "g_dense_stride", 9, 10)
    refused(bent(g_pq=DUMMY + 8), "backward", "g_pq", "16-byte")


def test_host_tensors_are_refused_without_a_fallback():
    ents = torch.zeros(2, 5, 31)
    items = torch.zeros(2, 8, 16)
    with pytest.raises(heads.HeadsError, match="runs on the GPU"):
        decoder.decoder_heads(torch.zeros(2, 3), torch.zeros(2, 2, 40), [ents, items], [-1, 0, 1], torch.ones(2, 18),
                              [3, 6, 9])


# ---------------------------------------------------------------- the yardstick (numpy)
def fma32(a, b, c):
    """float32 fmaf(a, b, c): the product of two float32 is exact in float64, the sum is rounded once to
    the 64-bit mantissa of a long double and then to float32 (a second rounding that matters only on an
    exact tie of the first, which the long double's 40 extra bits make vanishingly rare)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.longdouble)).astype(F32)


def class_of(v, hi):
    """clamp(trunc(v), 0, hi), NaN -> 0"""
    with np.errstate(invalid="ignore"):
        return np.where(v >= 0, np.minimum(np.trunc(np.nan_to_num(v, nan=0.0)), hi), 0).astype(np.int64)


def spec_item_logit(pq, x):
    """SPEC §20 on pq [N, >= 33] and items x [N, R, 16], float32 term by term: [N, R]."""
    pq, x = pq.astype(F32), x.astype(F32)
    rows = np.arange(pq.shape[0])[:, None]
    v = (pq[:, 32:33] + pq[rows, class_of(x[:, :, 1], 17)]).astype(F32)
    v = (v + pq[rows, 18 + class_of(x[:, :, 14], 1)]).astype(F32)
    with np.errstate(invalid="ignore"):
        for k, col in enumerate(item.CONT_COLS):
            v = fma32(pq[:, 20 + k:21 + k], (x[:, :, col] * F32(0.01)).astype(F32), v)
    return v


def spec_entity_logit(pq, x):
    """SPEC §21 on pq [N, >= 36] and entities x [N, R, 31], float32 term by term: [N, R]."""
    pq, x = pq.astype(F32), x.astype(F32)
    rows = np.arange(pq.shape[0])[:, None]
    v = (pq[:, 35:36] + pq[rows, 1 + class_of(x[:, :, 1], 4)]).astype(F32)
    with np.errstate(invalid="ignore"):
        v = fma32(pq[:, 0:1], x[:, :, 0], v)
        for k in range(29):
            v = fma32(pq[:, 6 + k:7 + k], x[:, :, 2 + k], v)
    return v


def spec_decoder_tile(dense, pq, sets, rules, head_set, legal, dims):
    """SPEC §23's staged tile [N, sum(dims)] float32: head k's entries at its offset, -inf wherever the
    mask forbids; a dense head's given logit, a pointer head's §20 / §21 value for j < R and 0.0 for the
    no-op. dense [N, D], pq [N, P, 40], sets[s] [N, R_s, cols] (already one per row), legal bool."""
    n = legal.shape[0]
    tile = np.full((n, int(sum(dims))), -np.inf, dtype=F32)
    off, d, p = 0, 0, 0
    for k, size in enumerate(dims):
        s = head_set[k]
        if s < 0:
            x = dense[:, d:d + size].astype(F32)
            d += size
        else:
            fn = spec_item_logit if rules[s] == decoder.SET_ITEM else spec_entity_logit
            x = np.concatenate([fn(pq[:, p], sets[s]), np.zeros((n, 1), F32)], 1)
            p += 1
        m = legal[:, off:off + size]
        tile[:, off:off + size][m] = x[m]
        off += size
    return tile


def composed_tile(dense, q, enc_item, enc_player, sets, rules, head_set, legal, dims, dtype):
    """The same tile from torch's composed expressions on the CPU: features_ref, pointer_query, a product
    and a sum, 0 for the no-op, a masked fill of -inf. q [N, P, H] are the heads' raw queries."""
    parts, d, p = [], 0, 0
    for k, size in enumerate(dims):
        s = head_set[k]
        if s < 0:
            parts.append(dense[:, d:d + size].to(dtype))
            d += size
            continue
        if rules[s] == decoder.SET_ITEM:
            x, pq = item.item_features_ref(sets[s].to(dtype)), enc_item.pointer_query(q[:, p:p + 1].to(dtype))[:, 0]
        else:
            x, pq = player.player_features_ref(sets[s].to(dtype)), enc_player.pointer_query(q[:, p:p + 1].to(dtype))[:, 0]
        f = x.shape[-1]
        lg = (torch.nan_to_num(x, nan=0.0) * pq[:, None, :f]).sum(-1) + pq[:, f:f + 1]
        parts.append(torch.cat([lg, lg.new_zeros(lg.shape[0], 1)], 1))
        p += 1
    return torch.cat(parts, 1).masked_fill(~torch.from_numpy(legal), float("-inf"))


def tile_inputs(exact, seed=4, n=7, hidden=16):
    """Generated rows of three entity heads over 100, four item heads over 12 and one over 65, and two
    dense heads, with `hidden`-wide encoders. exact: every partial sum of every logit is exact."""
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    dims, head_set = [3, 101, 66, 13, 13, 101, 9, 101, 13, 13], [-1, 0, 2, 1, 1, 0, -1, 0, 1, 1]
    rules = [decoder.SET_ENTITY, decoder.SET_ITEM, decoder.SET_ITEM]
    ents = make_entity_sets(n, 100, rng, nan=False)[0]
    sets = [ents, make_item_sets(n, 12, rng, nan=False), make_item_sets(n, 65, rng, nan=False)]
    enc_item, enc_player = item.ItemEncoder(hidden), player.PlayerEncoder(hidden, hidden)
    n_ptr = sum(s >= 0 for s in head_set)
    if exact:  # queries that pick one row of W each: pq = (W[i], b[i]) exactly, W and b small integers
        with torch.no_grad():
            enc_player.agent_fc.weight.copy_(torch.randint(-3, 4, enc_player.agent_fc.weight.shape).float())
            enc_player.agent_fc.bias.copy_(torch.randint(-3, 4, enc_player.agent_fc.bias.shape).float())
            w = torch.randint(-3, 4, enc_item.fc.weight.shape).float()
            w[:, 20:] = 0  # x[20 + k] = col * 0.01f has a full mantissa: no sum with it is exact in any order
            enc_item.fc.weight.copy_(w)
            enc_item.fc.bias.copy_(torch.randint(-3, 4, enc_item.fc.bias.shape).float())
        q = torch.zeros(n, n_ptr, hidden)
        q[torch.arange(n)[:, None], torch.arange(n_ptr)[None, :], torch.randint(0, hidden, (n, n_ptr))] = 1.0
        dense = torch.randint(-5, 6, (n, 12)).float()
    else:
        q = torch.randn(n, n_ptr, hidden)
        dense = torch.randn(n, 12)
    legal = rng.random((n, sum(dims))) < 0.4
    legal[0], legal[1] = False, True
    return dims, head_set, rules, [torch.from_numpy(s) for s in sets], enc_item, enc_player, q, dense, legal


def fold(q, head_set, rules, enc_item, enc_player):
    """pq [N, P, 40] float32 of the raw queries, as `BaselineAgent.pointer_slots` lays it out."""
    out = []
    with torch.no_grad():
        for p, s in enumerate(s for s in head_set if s >= 0):
            pq = (enc_item if rules[s] == decoder.SET_ITEM else enc_player).pointer_query(q[:, p:p + 1])[:, 0]
            out.append(torch.cat([pq, pq.new_zeros(pq.shape[0], 40 - pq.shape[1])], 1))
    return torch.stack(out, 1).numpy()


def test_spec_decoder_tile_equals_the_composed_expressions_where_sums_are_exact():
    dims, head_set, rules, sets, enc_item, enc_player, q, dense, legal = tile_inputs(exact=True)
    pq = fold(q, head_set, rules, enc_item, enc_player)
    got = spec_decoder_tile(dense.numpy(), pq, [s.numpy() for s in sets], rules, head_set, legal, dims)
    with torch.no_grad():
        want = composed_tile(dense, q, enc_item, enc_player, sets, rules, head_set, legal, dims, torch.float32).numpy()
    assert got.dtype == F32 and got.shape == (7, sum(dims))
    assert np.array_equal(np.isneginf(got), ~legal)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    off = np.cumsum([0] + dims)
    for k, s in enumerate(head_set):  # the no-op entries are +0.0 where legal, and some logit is not 0
        if s >= 0:
            noop = got[:, off[k + 1] - 1]
            assert np.all(noop[legal[:, off[k + 1] - 1]] == 0)
            assert np.any(got[:, off[k]:off[k + 1] - 1][legal[:, off[k]:off[k + 1] - 1]] != 0), k


def test_spec_decoder_tile_stays_within_its_roundings_of_the_float64_chain():
    dims, head_set, rules, sets, enc_item, enc_player, q, dense, legal = tile_inputs(exact=False)
    pq = fold(q, head_set, rules, enc_item, enc_player)
    got = spec_decoder_tile(dense.numpy(), pq, [s.numpy() for s in sets], rules, head_set, legal, dims)
    # float64 from the float32 pq the kernel is given: what is bounded is the chain, not the fold
    off, p = np.cumsum([0] + dims), 0
    for k, s in enumerate(head_set):
        if s < 0:
            continue
        x64 = (item.item_features_ref if rules[s] == decoder.SET_ITEM else player.player_features_ref)(sets[s].double())
        f = x64.shape[-1]
        terms = x64.numpy() * pq[:, p, None, :f].astype(np.float64)
        want = terms.sum(-1) + pq[:, p, f:f + 1]
        # x[20 + k] = col * 0.01f is itself rounded once: one more rounding per scaled term
        bound = (f + 1 + 12) * EPS * (np.abs(terms).sum(-1) + np.abs(pq[:, p, f:f + 1])) * 1.01
        m = legal[:, off[k]:off[k + 1] - 1]
        err = np.abs(got[:, off[k]:off[k + 1] - 1].astype(np.float64) - want)
        assert np.all(err[m] <= bound[m]), (k, float(err[m].max()), float(bound[m].min()))
        assert err[m].max() > 0  # (general weights: the comparison is not vacuous)
        p += 1
