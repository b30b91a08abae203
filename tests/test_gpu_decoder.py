"""The decoder kernels (nmmo_amd/decoder.py, csrc/decoder.hip, SPEC.md §23) on MI355X.

The yardstick is the composition the repository already has, on the same inputs: `item_logits` per item
set, `player_logits` per entity set, `cat` with the dense heads' logits, `masked_heads_full` with the
same seed / offset / row_base, and autograd through all of it. Every output and both gradients are
compared with `torch.equal` on their bits (`same_bits`): no tolerance appears in this comparison.
§23 derives the equality: the same device functions on the same values in the same order, without
contraction.

The float64 anchors at the end are not self-consistency checks: logprob, entropy, the sampled actions
and the gradients with respect to the queries and the dense logits are compared with
test_gpu_heads.py's float64 closed form on float64 logits built from float64 features and weights,
within 4 x the error of the unfused float32 torch chain (embeddings, zero row, `matmul`,
`Categorical`) against the same values (`within`).

Shapes. The nmmo heads over flat rows of 23,987 floats, sets read in place (the sections lie at every
alignment mod 16 bytes). Synthetic A: entity sets of 65 and 256, item sets of 1 and 64, two heads on one
set. Synthetic B: item sets of 65 and 1,024. Synthetic C: 700 dense entries, an item set of 1,024 and an
entity set of 256, whose 16,696 bytes of LDS a wave make the launch take two rows per workgroup. These
are the chunk (64 listed entities, 64 lanes of listed items) and path boundaries. Row counts 1, 3, 5, 37:
a partial workgroup, a full one and a partial, a prime count.

Mask rows: row 0 and rows >= 5 give head k of row r a legal count from (0, 1, 8, 64, 65, R) by
(r + k) % 6, at random places, the no-op legal unless (r + k) % 3 == 0; row 1 all illegal (every head
empty: a sampled action is uniform); row 2 all legal (all 100 entities, all 1,024 listings); row 3 the
no-op alone; row 4 the no-op illegal and the first and 30 % of the other candidates legal. Row 6's second head is given an
illegal action while it has legal entries."""

import ctypes
import types

import numpy as np
import pytest
import torch

from tests.conftest import gpu_available
from tests.test_gpu_heads import check_samples, closed_form, closed_grad, head_slices, within
from tests.test_gpu_item import make_sets as make_item_sets
from tests.test_gpu_player import make_sets as make_entity_sets, same_bits

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

DEV = "cuda"
ROW = 23987
E, I = 0, 1  # decoder.SET_ENTITY, decoder.SET_ITEM
COLS = {E: 31, I: 16}
NMMO_DIMS = [3, 101, 1025, 13, 13, 101, 99, 101, 5, 13, 99, 13]
CONFIGS = {
    # name: (dims, head_set, rules, rows)
    "nmmo": (NMMO_DIMS, [-1, 0, 2, 1, 1, 0, -1, 0, -1, 1, -1, 1], [E, I, I], [100, 12, 1024]),
    "A": ([3, 66, 257, 2, 65, 66, 5], [-1, 0, 1, 2, 3, 0, -1], [E, E, I, I], [65, 256, 1, 64]),
    "B": ([5, 66, 1025, 66, 7], [-1, 0, 1, 0, -1], [I, I], [65, 1024]),
    "C": ([700, 1025, 257], [-1, 0, 1], [I, E], [1024, 256]),
}
ROWS = [1, 3, 5, 37]
SEED, OFFSET, ROW_BASE = 0x1234_5678_9ABC, 7, 0xFFFF_FFF0  # row_base + r wraps past 2^32


class Case:
    def __init__(self, name, n, seed=0):
        from nmmo_amd import layout

        rng = np.random.default_rng(1000 * sum(map(ord, name)) + 10 * n + seed)
        self.name, self.n = name, n
        self.dims, self.head_set, self.rules, self.rows = CONFIGS[name]
        self.total, self.slices = sum(self.dims), head_slices(self.dims)
        self.pointer = [k for k, s in enumerate(self.head_set) if s >= 0]
        self.n_dense = sum(d for d, s in zip(self.dims, self.head_set) if s < 0)
        if name == "nmmo":
            lay = layout.flat_layout(2048)
            self.off = [lay[sec].offset for sec in ("Entity", "Inventory", "Market")]
            self.stride = ROW
            assert layout.obs_elems(2048) == ROW and sorted({r * ROW * 4 % 16 for r in range(4)}) == [0, 4, 8, 12]
        else:
            self.off, o = [], self.total + 3
            for s, R in enumerate(self.rows):
                self.off.append(o)
                o += COLS[self.rules[s]] * R + 5
            self.stride = max(ROW, o | 1)
        # ---- the candidates: integer-valued, so the int16 copy holds the same values
        self.sets_np = [make_entity_sets(n, R, rng, nan=False)[0] if rule == E else make_item_sets(n, R, rng, nan=False)
                        for rule, R in zip(self.rules, self.rows)]
        # ---- the mask
        legal = np.zeros((n, self.total), dtype=bool)
        counts = {}
        for r in range(n):
            for k, sl in enumerate(self.slices):
                size = sl.stop - sl.start
                if r == 1:
                    continue
                if r == 2:
                    legal[r, sl] = True
                elif r == 3:
                    legal[r, sl.stop - 1] = True
                elif r == 4:
                    legal[r, sl.start:sl.stop - 1] = rng.random(size - 1) < 0.3
                    legal[r, sl.start] = size > 1
                else:
                    m = size - 1 if self.head_set[k] >= 0 else size
                    c = min(m, (0, 1, 8, 64, 65, m)[(r + k) % 6])
                    legal[r, sl.start + rng.choice(m, c, replace=False)] = True
                    if self.head_set[k] >= 0:
                        legal[r, sl.stop - 1] = (r + k) % 3 != 0
                    counts.setdefault(k, set()).add(c)
        self.legal, self.counts = legal, counts
        buf = rng.integers(-9, 9, (n, self.stride)).astype(np.float32)
        buf[:, :self.total] = np.where(legal, rng.choice([1.0, 0.5, 3.0], legal.shape), rng.choice([0.0, -1.0], legal.shape))
        for s, x in enumerate(self.sets_np):
            buf[:, self.off[s]:self.off[s] + x[0].size] = x.reshape(n, -1)
        self.buf = torch.from_numpy(buf).to(DEV)
        self.ibuf = torch.from_numpy(buf.astype(np.int16)).to(DEV)  # the same sections as int16 (the prefix is junk)
        self.mask_u8 = torch.zeros((n, self.total + 5), dtype=torch.uint8, device=DEV)
        self.mask_u8[:, :self.total] = torch.from_numpy(legal).to(DEV).to(torch.uint8) * 3
        self.keep = (self.buf.clone(), self.ibuf.clone(), self.mask_u8.clone())
        # ---- queries, dense logits, given actions, incoming gradients
        pq = rng.standard_normal((n, len(self.pointer), 40)).astype(np.float32)
        for p, k in enumerate(self.pointer):  # logits of a few units: raw entity columns reach 3,000
            if self.rules[self.head_set[k]] == E:
                pq[:, p, 0], pq[:, p, 6:35] = pq[:, p, 0] * 2.0 ** -12, pq[:, p, 6:35] * 2.0 ** -12
            else:
                pq[:, p, 20:32] *= 2.0 ** -4
        self.pq = torch.from_numpy(pq).to(DEV)
        self.dense = torch.from_numpy(rng.standard_normal((n, self.n_dense)).astype(np.float32)).to(DEV)
        actions = np.zeros((n, len(self.dims)), dtype=np.int64)
        for r in range(n):
            for k, sl in enumerate(self.slices):
                idx = np.flatnonzero(legal[r, sl])
                actions[r, k] = rng.choice(idx) if len(idx) else rng.integers(sl.stop - sl.start)
        self.illegal = None
        if n > 6:  # (6 + 1) % 6 = 1: one legal candidate and the no-op
            sl = self.slices[1]
            bad = np.flatnonzero(~legal[6, sl])
            assert legal[6, sl].any() and len(bad)
            actions[6, 1] = bad[0]
            self.illegal = (6, 1)
        self.actions = torch.from_numpy(actions).to(DEV)
        self.g_logprob = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV)
        self.g_entropy = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV)

    def view(self, s, buf=None):
        """Set s as a view of the rows: read in place."""
        buf = self.buf if buf is None else buf
        return buf[:, self.off[s]:self.off[s] + COLS[self.rules[s]] * self.rows[s]]

    def unchanged(self):
        now = (self.buf, self.ibuf, self.mask_u8)
        return all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                               b.view(torch.int32) if b.dtype == torch.float32 else b) for a, b in zip(now, self.keep))

    # ---- the two paths; `buf` holds the sets, `mask` the mask rows
    def fused(self, dense, pq, action=None, buf=None, mask=None, share=None):
        from nmmo_amd.decoder import decoder_heads_full

        sets = [(self.view(s, buf), "entity" if rule == E else "item", 1 if share is None else share[s])
                for s, rule in enumerate(self.rules)]
        return decoder_heads_full(dense, pq, sets, self.head_set, self.buf if mask is None else mask, self.dims, action,
                                  seed=SEED, offset=OFFSET, row_base=ROW_BASE)

    def composed(self, dense, pq, action=None, buf=None, mask=None, keep=None):
        from nmmo_amd.heads import masked_heads_full
        from nmmo_amd.item import item_logits
        from nmmo_amd.player import player_logits

        mask = self.buf if mask is None else mask
        parts, d = [None] * len(self.dims), 0
        for k, s in enumerate(self.head_set):
            if s < 0:
                parts[k] = dense[:, d:d + self.dims[k]]
                d += self.dims[k]
        for s, (rule, R) in enumerate(zip(self.rules, self.rows)):
            ks = [k for k in self.pointer if self.head_set[k] == s]
            idx, width = [self.pointer.index(k) for k in ks], 40 if rule == E else 36
            slots = pq[:, idx, :width]
            if keep is not None:  # a leaf: its .grad is the *_logits_backward kernel's output, untouched
                slots = slots.detach().requires_grad_(True)
                keep.setdefault("slots", []).append((idx, width, slots))
            fn = player_logits if rule == E else item_logits
            lg = fn(self.view(s, buf), slots, mask, [self.slices[k].start for k in ks], set_rows=R)
            for i, k in enumerate(ks):
                parts[k] = lg[:, i * (R + 1):(i + 1) * (R + 1)]
        logits = torch.cat(parts, 1)
        if keep is not None:
            logits.retain_grad()  # nmh_backward's output, untouched
            keep["logits"] = logits
        return masked_heads_full(logits, mask, self.dims, action, seed=SEED, offset=OFFSET, row_base=ROW_BASE)

    def grads(self, path, use_lp, use_ent, **kw):
        """(the five outputs at the given actions, g_dense, g_pq) of `path`. The composed path's gradients
        are read where its kernels wrote them (the logits' gradient, each set's slots' gradient) and copied
        into place: autograd's own sums over the slices would turn a kernel's -0.0 into +0.0."""
        dense, pq = self.dense.clone().requires_grad_(True), self.pq.clone().requires_grad_(True)
        keep = {} if path == self.composed else None
        if keep is not None:
            kw = dict(kw, keep=keep)
        out = path(dense, pq, self.actions, **kw)
        loss = 0.0
        if use_lp:
            loss = loss + (out[1] * self.g_logprob).sum()
        if use_ent:
            loss = loss + (out[2] * self.g_entropy).sum()
        loss.backward()
        if keep is None:
            return [t.detach() for t in out], dense.grad, pq.grad
        g = keep["logits"].grad
        g_dense = torch.cat([g[:, sl] for sl, s in zip(self.slices, self.head_set) if s < 0], 1)
        g_pq = torch.zeros_like(pq)
        for idx, width, slots in keep["slots"]:
            g_pq[:, idx, :width] = slots.grad
        return [t.detach() for t in out], g_dense, g_pq


_cases = {}


def case(name, n):
    if (name, n) not in _cases:
        _cases[(name, n)] = Case(name, n)
    return _cases[(name, n)]


def same(a, b):
    return same_bits(a, b) if a.dtype == torch.float32 else (a.dtype == b.dtype and torch.equal(a, b))


def assert_same_outputs(got, want, what):
    for name, a, b in zip(("action", "logprob", "entropy", "lse", "head_entropy"), got, want):
        assert same(a, b), (what, name)


# ---------------------------------------------------------------- 1. bit for bit the composed path
def test_the_cases_hold_the_rows_the_kernels_can_go_wrong_on():
    c = case("nmmo", 37)
    assert c.counts[1] >= {64, 65, 100} and c.counts[5] >= {0, 1, 8} and c.counts[2] == {0, 1, 8, 64, 65, 1024}
    assert not c.legal[1].any() and c.legal[2].all() and c.illegal == (6, 1)
    for k in c.pointer:
        sl = c.slices[k]
        assert c.legal[3, sl].sum() == 1 and c.legal[3, sl.stop - 1]
        assert not c.legal[4, sl.stop - 1] and c.legal[4, sl].any()
    assert case("A", 37).counts[2] >= {64, 65, 256} and case("C", 37).counts[1] == {0, 1, 8, 64, 65, 1024}


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_forward_equals_the_composed_path_bit_for_bit(name, n):
    c = case(name, n)
    with torch.no_grad():
        got, want = c.fused(c.dense, c.pq), c.composed(c.dense, c.pq)
        assert got[0].dtype == torch.int32 and tuple(got[0].shape) == (n, len(c.dims))
        assert_same_outputs(got, want, "sampling")
        got, want = c.fused(c.dense, c.pq, c.actions), c.composed(c.dense, c.pq, c.actions)
        assert got[0] is c.actions
        assert_same_outputs(got, want, "given")
        if c.illegal:
            assert float(got[1][c.illegal[0]]) < -9e8  # masked_fill(-1e9)'s logprob
        if n > 1:
            assert torch.all(got[3][1] == 0) and torch.all(got[4][1] == 0) and float(got[1][1]) == 0  # every head empty
    assert c.unchanged()


@pytest.mark.parametrize("use_lp,use_ent", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_backward_equals_the_composed_path_bit_for_bit(name, n, use_lp, use_ent):
    c = case(name, n)
    out, g_dense, g_pq = c.grads(c.fused, use_lp, use_ent)
    out_w, g_dense_w, g_pq_w = c.grads(c.composed, use_lp, use_ent)
    assert_same_outputs(out, out_w, "given")
    assert same_bits(g_dense, g_dense_w) and same_bits(g_pq, g_pq_w)
    assert torch.isfinite(g_pq).all() and torch.isfinite(g_dense).all()
    if n > 5:
        assert float(g_pq.abs().max()) > 0 and float(g_dense.abs().max()) > 0
    for p, k in enumerate(c.pointer):  # the floats of a slot that forward ignores
        used = 36 if c.rules[c.head_set[k]] == E else 33
        assert torch.all(g_pq[:, p, used:].view(torch.int32) == 0)
    assert c.unchanged()


def test_a_gradient_nothing_requires_is_not_computed():
    c = case("nmmo", 5)
    dense, pq = c.dense.clone().requires_grad_(True), c.pq.clone()
    out = c.fused(dense, pq, c.actions)
    (out[1] * c.g_logprob).sum().backward()
    want = c.grads(c.fused, True, False)
    assert same_bits(dense.grad, want[1])
    dense, pq = c.dense.clone(), c.pq.clone().requires_grad_(True)
    out = c.fused(dense, pq, c.actions)
    (out[2] * c.g_entropy).sum().backward()
    assert same_bits(pq.grad, c.grads(c.fused, False, True)[2])


# ---------------------------------------------------------------- 2. kinds, poison, canaries, sharing
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_element_and_mask_kinds_give_identical_bits(name):
    c = case(name, 5)
    want = c.grads(c.fused, True, True)
    for buf, mask in ((c.buf, c.mask_u8), (c.ibuf, c.buf), (c.ibuf, c.mask_u8)):
        got = c.grads(c.fused, True, True, buf=buf, mask=mask)
        assert_same_outputs(got[0], want[0], (buf.dtype, mask.dtype))
        assert same_bits(got[1], want[1]) and same_bits(got[2], want[2])
        with torch.no_grad():
            assert_same_outputs(c.fused(c.dense, c.pq, buf=buf, mask=mask), c.fused(c.dense, c.pq), "sampling")
    assert c.unchanged()


@pytest.mark.parametrize("name", ["nmmo", "A", "C"])
def test_candidates_no_head_allows_are_never_used(name):
    """Their columns are NaN (float32) or +-32,767 (int16): the outputs equal the unpoisoned run's."""
    c = case(name, 37)
    want = c.grads(c.fused, True, True)
    with torch.no_grad():
        want_s = c.fused(c.dense, c.pq)
    for buf, poison in ((c.buf.clone(), float("nan")), (c.ibuf.clone(), None)):
        hit = 0
        for s, (rule, R) in enumerate(zip(c.rules, c.rows)):
            heads_of = [k for k in c.pointer if c.head_set[k] == s]
            # (an entity set's kernels read a candidate any head of the set allows: poison where none does)
            dead = ~np.stack([c.legal[:, c.slices[k].start:c.slices[k].start + R] for k in heads_of]).any(0)  # [n, R]
            sec = c.view(s, buf).view(c.n, R, COLS[rule])  # a view: the assignment lands in buf
            fill = torch.full((COLS[rule],), poison if poison is not None else 0, dtype=buf.dtype, device=DEV)
            if poison is None:
                fill[0::2], fill[1::2] = 32767, -32767
            sec[torch.from_numpy(dead).to(DEV)] = fill
            hit += int(dead.sum())
        assert hit > c.n
        got = c.grads(c.fused, True, True, buf=buf)
        assert_same_outputs(got[0], want[0], buf.dtype)
        assert same_bits(got[1], want[1]) and same_bits(got[2], want[2])
        with torch.no_grad():
            assert_same_outputs(c.fused(c.dense, c.pq, buf=buf), want_s, buf.dtype)


def margined(shape, dtype, fill, margin=24):
    """(a tensor of `shape` inside a larger canary-filled buffer, the buffer, the window's bounds)."""
    count = int(np.prod(shape))
    whole = torch.full((count + 2 * margin,), fill, dtype=dtype, device=DEV)
    return whole[margin:margin + count].view(shape), whole, (margin, margin + count)


def margins_intact(whole, bounds, fill):
    lo, hi = bounds
    edge = torch.cat([whole[:lo], whole[hi:]])
    return bool(torch.isnan(edge).all()) if fill != fill else bool((edge == fill).all())


@pytest.mark.parametrize("name", ["nmmo", "C"])
def test_outputs_stay_inside_their_buffers_and_every_entry_is_written(name):
    from nmmo_amd import decoder, heads, item, player

    c = case(name, 5)
    n, nh, P = c.n, len(c.dims), len(c.pointer)
    hd = heads.heads_struct(c.dims)
    views = [c.view(s) for s in range(len(c.rules))]
    args = [(item._item_arg if rule == I else player._ent_arg)(v, R) for v, rule, R in zip(views, c.rules, c.rows)]
    assert all(a[0].data_ptr() == v.data_ptr() for a, v in zip(args, views))  # read in place
    st = decoder.sets_struct(c.head_set, c.rules, c.rows, [1] * len(c.rules), [a[1] for a in args],
                             [v.data_ptr() for v in views], decoder.ELEM_F32)
    nan = float("nan")
    outs = {"a": margined((n, nh), torch.int32, -77), "lp": margined((n,), torch.float32, nan),
            "ent": margined((n,), torch.float32, nan), "lse": margined((n, nh), torch.float32, nan),
            "hent": margined((n, nh), torch.float32, nan)}
    a_in = c.actions.to(torch.int32)
    common = [ctypes.byref(hd), ctypes.byref(st), n, c.pq.data_ptr(), c.dense.data_ptr(), c.n_dense, c.buf.data_ptr(),
              c.stride, heads.MASK_F32]
    heads.check(heads.lib().nmh_decoder_forward(*common, a_in.data_ptr(), SEED, OFFSET, ROW_BASE,
                                                *[outs[k][0].data_ptr() for k in ("a", "lp", "ent", "lse", "hent")],
                                                heads._stream()), "nmh_decoder_forward")
    torch.cuda.synchronize()
    for k, (t, whole, bounds) in outs.items():
        assert margins_intact(whole, bounds, -77 if k == "a" else nan), k
        assert not torch.isnan(t.float()).any() and (k != "a" or torch.equal(t, a_in)), k
    with torch.no_grad():
        want = c.fused(c.dense, c.pq, c.actions)
    assert same_bits(outs["lp"][0], want[1]) and same_bits(outs["lse"][0], want[3])
    # backward: g_dense rows 7 floats wider than the dense heads, g_pq inside margins (16-byte aligned)
    gs = c.n_dense + 7
    g_dense = torch.full((n, gs), nan, dtype=torch.float32, device=DEV)
    g_pq, whole, bounds = margined((n, P, 40), torch.float32, nan)
    assert g_pq.data_ptr() % 16 == 0
    heads.check(heads.lib().nmh_decoder_backward(*common, a_in.data_ptr(), outs["lse"][0].data_ptr(),
                                                 outs["hent"][0].data_ptr(), c.g_logprob.data_ptr(),
                                                 c.g_entropy.data_ptr(), g_dense.data_ptr(), gs, g_pq.data_ptr(),
                                                 heads._stream()), "nmh_decoder_backward")
    torch.cuda.synchronize()
    assert margins_intact(whole, bounds, nan)
    assert not torch.isnan(g_dense[:, :c.n_dense]).any() and torch.isnan(g_dense[:, c.n_dense:]).all()
    assert not torch.isnan(g_pq).any()
    want = c.grads(c.fused, True, True)
    assert same_bits(g_dense[:, :c.n_dense].contiguous(), want[1]) and same_bits(g_pq.contiguous(), want[2])
    assert c.unchanged()


def test_a_call_allocates_its_outputs_and_nothing_else():
    c = case("nmmo", 37)
    a_in = c.actions.to(torch.int32)
    with torch.no_grad():
        c.fused(c.dense, c.pq, a_in)  # (warm: the library is loaded)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = c.fused(c.dense, c.pq, a_in)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    n, nh = c.n, len(c.dims)
    sizes = [n * nh * 4] * 3 + [n * 4] * 2  # actions_out, lse, head_entropy; logprob, entropy
    assert peak <= sum((s + 511) // 512 * 512 for s in sizes), peak  # the caching allocator's 512-byte blocks
    del out


def test_native_sharing_reads_one_market_for_the_rows_of_an_env():
    """share = 4 over one int16 Market per env for 8 rows equals share = 1 over the expanded copy."""
    from nmmo_amd.decoder import decoder_heads_full

    rng = np.random.default_rng(5)
    n, share, R = 8, 4, 1024
    dims, head_set = [5, R + 1], [-1, 0]
    market = torch.from_numpy(make_item_sets(n // share, R, rng, nan=False).astype(np.int16)).to(DEV)  # [2, 1024, 16]
    expanded = market.repeat_interleave(share, 0).contiguous()
    legal = rng.random((n, sum(dims))) < 0.1
    mask = torch.from_numpy(legal).to(DEV)
    pq = torch.from_numpy(rng.standard_normal((n, 1, 40)).astype(np.float32)).to(DEV)
    pq[:, :, 20:32] *= 2.0 ** -4
    dense = torch.from_numpy(rng.standard_normal((n, 5)).astype(np.float32)).to(DEV)
    res = []
    for sets in ([(market, "item", share)], [(expanded, "item", 1)]):
        d, q = dense.clone().requires_grad_(True), pq.clone().requires_grad_(True)
        out = decoder_heads_full(d, q, sets, head_set, mask, dims, seed=3, offset=1)
        given = decoder_heads_full(d, q, sets, head_set, mask, dims, out[0], seed=3, offset=1)
        (given[1].sum() + 0.5 * given[2].sum()).backward()
        res.append((out, given, d.grad, q.grad))
    assert_same_outputs(res[0][0], res[1][0], "sampling")
    assert_same_outputs(res[0][1][1:], res[1][1][1:], "given")
    assert same_bits(res[0][2], res[1][2]) and same_bits(res[0][3], res[1][3])
    assert float(res[0][3].abs().max()) > 0
    # rows of one env with the same mask and query would agree; rows of different envs read different markets
    assert not torch.equal(market[0], market[1])


# ---------------------------------------------------------------- 3. anchors against float64
class Anchor:
    """The nmmo heads with queries that come from encoders, so that the unfused float32 chain exists:
    ItemEncoder / PlayerEncoder of width 16, raw queries q [N, 8, 16], pq = pointer_query(q)."""

    def __init__(self, n):
        from nmmo_amd.item import ItemEncoder
        from nmmo_amd.player import PlayerEncoder

        c = self.c = case("nmmo", n)
        torch.manual_seed(n)
        self.enc = {I: ItemEncoder(16).to(DEV), E: PlayerEncoder(16, 16).to(DEV)}
        with torch.no_grad():  # logits of a few units from raw columns up to 32,767
            self.enc[E].agent_fc.weight.mul_(2.0 ** -12)
            self.enc[I].fc.weight[:, 20:].mul_(2.0 ** -3)
        self.q = torch.randn(n, len(c.pointer), 16, device=DEV)
        self.sets = [torch.from_numpy(x).to(DEV) for x in c.sets_np]

    def slots(self, q):
        c = self.c
        out = []
        for p, k in enumerate(c.pointer):
            pq = self.enc[c.rules[c.head_set[k]]].pointer_query(q[:, p:p + 1])[:, 0]
            out.append(torch.cat([pq, pq.new_zeros(c.n, 40 - pq.shape[1])], 1))
        return torch.stack(out, 1)

    def chain(self, dense, q, dtype):
        """The reference's logits [N, 1586] in `dtype`: embeddings, zero row, matmul."""
        from nmmo_amd.item import item_features_ref
        from nmmo_amd.player import player_features_ref

        c, parts, d, emb = self.c, [], 0, []
        for s, rule in enumerate(c.rules):
            enc = self.enc[rule]
            fc = enc.fc if rule == I else enc.agent_fc
            x = (item_features_ref if rule == I else player_features_ref)(self.sets[s].to(dtype))
            e = torch.nn.functional.linear(x, fc.weight.to(dtype), fc.bias.to(dtype))
            emb.append(torch.cat([e, e.new_zeros(c.n, 1, e.shape[2])], 1))
        p = 0
        for k, s in enumerate(c.head_set):
            if s < 0:
                parts.append(dense[:, d:d + c.dims[k]].to(dtype))
                d += c.dims[k]
            else:
                parts.append(torch.matmul(emb[s], q[:, p].to(dtype).unsqueeze(-1)).squeeze(-1))
                p += 1
        return torch.cat(parts, 1)


_anchors = {}


def anchor(n):
    if n not in _anchors:
        _anchors[n] = Anchor(n)
    return _anchors[n]


@pytest.mark.parametrize("n", [5, 37])
def test_logprob_entropy_and_samples_against_the_float64_closed_form(n):
    from tests.test_gpu_heads import torch_heads

    a = anchor(n)
    c = a.c
    with torch.no_grad():
        x64 = a.chain(c.dense, a.q, torch.float64).cpu().numpy()
        want = closed_form(x64, c.legal, c.dims, c.actions.cpu().numpy())
        ref = [t.double().cpu().numpy() for t in torch_heads(a.chain(c.dense, a.q, torch.float32), c.buf, c.dims, c.actions)]
        got = c.fused(c.dense, a.slots(a.q), c.actions)
        sampled = c.fused(c.dense, a.slots(a.q))
    rows = np.ones(n, dtype=bool)
    if c.illegal:
        rows[c.illegal[0]] = False  # a logprob near -1e9, where one float32 ulp is 64: an E_ref of its own
        within("logprob (illegal action)", got[1].cpu().numpy(), want[0], ref[0], rows=~rows)
    within("logprob", got[1].cpu().numpy(), want[0], ref[0], rows=rows)
    within("entropy", got[2].cpu().numpy(), want[1], ref[1])
    within("lse", got[3].cpu().numpy(), want[2], ref[2])
    within("head entropy", got[4].cpu().numpy(), want[3], ref[3])
    shim = types.SimpleNamespace(name=f"decoder-{n}", n=n, dims=c.dims, slices=c.slices, legal=c.legal, logits_np=x64)
    check_samples(shim, sampled[0], SEED, OFFSET, ROW_BASE)


@pytest.mark.parametrize("use_lp,use_ent", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("n", [5, 37])
def test_gradients_against_the_float64_closed_form(n, use_lp, use_ent):
    from tests.test_gpu_heads import torch_heads

    a = anchor(n)
    c = a.c
    glp = c.g_logprob if use_lp else torch.zeros_like(c.g_logprob)
    gen = c.g_entropy if use_ent else torch.zeros_like(c.g_entropy)
    # float64: closed_grad gives d / d logits; the chain rule through the float64 logits gives d / d q, d / d dense
    dense64, q64 = c.dense.double().requires_grad_(True), a.q.double().requires_grad_(True)
    x64 = a.chain(dense64, q64, torch.float64)
    g = closed_grad(x64.detach().cpu().numpy(), c.legal, c.dims, c.actions.cpu().numpy(), glp.double().cpu().numpy(),
                    gen.double().cpu().numpy())
    x64.backward(torch.from_numpy(g).to(DEV))
    # the unfused float32 chain
    dense32, q32 = c.dense.clone().requires_grad_(True), a.q.clone().requires_grad_(True)
    logp, ent, _, _ = torch_heads(a.chain(dense32, q32, torch.float32), c.buf, c.dims, c.actions)
    ((logp * glp).sum() + (ent * gen).sum()).backward()
    # the kernels
    dense, q = c.dense.clone().requires_grad_(True), a.q.clone().requires_grad_(True)
    out = c.fused(dense, a.slots(q), c.actions)
    loss = 0.0
    if use_lp:
        loss = loss + (out[1] * c.g_logprob).sum()
    if use_ent:
        loss = loss + (out[2] * c.g_entropy).sum()
    loss.backward()
    f = lambda t: t.detach().double().cpu().numpy()  # noqa: E731
    within("g_dense", f(dense.grad), f(dense64.grad), f(dense32.grad))
    within("g_query", f(q.grad), f(q64.grad), f(q32.grad))
    assert np.abs(f(q64.grad)).max() > 0
