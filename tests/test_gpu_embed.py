"""The embedded-set kernels (nmmo_amd/csrc/embed_enc.hip, nmmo_amd/embed.py, SPEC.md §25) on MI355X.

Inputs are built as tests/test_gpu_player.py and tests/test_gpu_item.py build theirs: float32 sections
inside rows of 23,987 floats (so consecutive rows' sections lie at 0 / 12 / 8 / 4 bytes modulo 16) and
int16 sections at an odd offset of rows with an odd element stride. ENTITY: N in {1, 5, 9} rows with
R in {1, 63, 64, 65, 100, 256}; ITEM: R in {1, 12, 63, 64, 65, 1024} with share in {1, 3}. Columns hold
integers, +-32,767 among them; the discrete columns hold the values on each side of every clip edge
(`EDGES`; a case with at least 64 candidates holds all of them, which `Case` asserts) and, float32
only, NaN; about half the candidates are all zero and the middle set is all zero; the own-row cases
are test_gpu_player.py's.

- idx, cont and the own row: bit-equal to `embed_features_ref` on the GPU; counts exact.
- sums: equal to the float64 sums (the columns hold integers with |sum| < 2^24, so the float32 sum is
  exact in any order), and identical on two runs.
- logits: illegal and no-op entries exactly 0.0f. A legal entry is within (D + 2 C + 1) * 2^-24 *
  sum|terms| of float64 computed from the same float32 pq: D additions, C divisions and C fused
  multiply-adds in SPEC §25's order, each rounding once, at most 2^-24 of a partial sum that
  sum|terms| bounds to first order, and one more for the second-order terms. Candidates illegal in
  every head that reads them are NaN in every column and the outputs must be finite. A canary around
  every head's R + 1 entries stays untouched and the buffer is unchanged bitwise.
- logits_backward: within (cnt + 1) * 2^-24 * sum|terms| of float64 autograd through the materialised
  features (one rounding per legal candidate, the division's folded into the + 1 with the second
  order: a bin's sum has no other); pads 0; illegal and no-op entries of g_out are NaN and must not
  leak; identical on two runs.
- memory: a fused Market pass plus a Buy head stays below the [N, 1024, H] embedding's bytes, which
  the unfused path alone exceeds.
"""

import ctypes

import numpy as np
import pytest
import torch

from nmmo_amd import _sets, embed, heads
from nmmo_amd.embed import ENTITY, ITEM
from tests.conftest import gpu_available
from tests.test_gpu_heads import within

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

ROW = 23987  # floats of a flat obs row: rows' sections at 0 / 12 / 8 / 4 bytes mod 16
OFF = 4501   # the set's section of a synthetic row; the float masks of up to 4 heads lie in front
ID_OFF = 4400  # the row's AgentId element
F32, I16 = _sets.ELEM_F32, _sets.ELEM_I16
ENTITY_HEADS = {1: 4, 63: 3, 64: 4, 65: 3, 100: 3, 256: 4}
ITEM_HEADS = {1: 4, 12: 4, 63: 3, 64: 4, 65: 3, 1024: 2}
ENTITY_SHAPES = [(1, 1), (5, 63), (9, 64), (5, 65), (9, 100), (1, 100), (5, 256)]  # (N, R)
ITEM_SHAPES = [(1, 1, 1), (5, 12, 1), (9, 12, 3), (5, 63, 1), (9, 64, 3), (5, 65, 1), (5, 1024, 1), (9, 1024, 3)]
EPS = 2.0 ** -24
CANARY = 7.5
DEV = "cuda"
OWN_CASES = 7  # set m's own-row case is m % 7
# the values on each side of every clip edge, per discrete column
EDGES = {
    ENTITY.name: {0: [-32767, -1, 0, 1, 128, 255, 256, 32767], 1: [-257, -256, -255, -1, 0],
                  8: [-513, -512, -511, -258, -257, -256], 10: [-769, -768, -767, -514, -513, -512]},
    ITEM.name: {1: [-3, -2, -1, 0, 17, 253, 254], 14: [-1, 0, 1, 2, 255, 256]},
}


def ID_COL_ENTITY(kind):
    return embed.ID_COL if kind is ENTITY else -1


def make_sets(kind, m, R, rng, nan=True):
    """[m, R, cols] float32 integer-valued sets and (entity kind) the rows' ids [m]: about half the
    candidates all zero, the clip edges in the discrete columns, +-32,767 columns, the middle set all
    zero; an entity set m's id is placed for own-row case m % 7 (see `want_own`)."""
    cols = kind.cols
    x = rng.integers(-300, 3000, (m, R, cols)).astype(np.float32)
    if kind is ENTITY:
        ident = np.stack([rng.permutation(np.arange(1000, 1000 + R)) for _ in range(m)]).astype(np.float32)
        x[:, :, 0] = np.where(rng.random((m, R)) < 0.3, -ident, ident)
        x[:, :, 1] = rng.integers(0, 5, (m, R))
        x[:, :, 8] = np.where(rng.random((m, R)) < 0.5, 0, rng.integers(1, 129, (m, R)))
        x[:, :, 10] = rng.integers(0, 3, (m, R))
    else:
        x[:, :, 1] = rng.integers(0, 18, (m, R))
        x[:, :, 14] = rng.integers(0, 2, (m, R))
    x[rng.random((m, R)) < 0.5] = 0
    flat = x.reshape(m * R, cols)
    k = flat.shape[0]
    # the edge values: not in the middle set, which is zeroed, nor (entity column 0) where the own-row cases write
    j, keep = np.arange(k) % R, (np.arange(k) // R != m // 2) | (m == 1)
    own = (j == 0) | (j == R - 1) | (j == R // 2) | (j == R // 3)
    for col, vals in EDGES[kind.name].items():
        vals = vals + ([np.nan] if nan and col != ID_COL_ENTITY(kind) else [])
        pos = rng.permutation(np.nonzero(keep & ~own if col == ID_COL_ENTITY(kind) else keep)[0])[:len(vals)]
        flat[pos, col] = vals[:len(pos)]
    cont = list(kind.ccols)
    flat[(3 * k) // 4, cont] = ([32767, -32767] * 14)[:len(cont)]
    flat[k // 3, cont[-1]] = -32767
    if m > 1:
        x[m // 2] = 0
    ids = np.zeros(m, dtype=np.float32)
    if kind is ENTITY:
        for s in range(m):
            case = s % OWN_CASES
            if case == 0:      # a match at entity 0
                ids[s] = x[s, 0, 0] = 7
            elif case == 1:    # a match at entity R - 1
                ids[s] = x[s, R - 1, 0] = 8
            elif case == 2:    # two matches: the first wins (one match when R < 3)
                ids[s] = x[s, R // 2, 0] = x[s, R - 1, 0] = 9
            elif case == 3:    # no match
                ids[s] = 5000
            elif case == 4:    # id 0 among zero-id entities
                ids[s] = 0
                x[s, R // 3, 0] = 0
            elif case == 5:    # a negative NPC id, its positive twin in front of it (when R > 1)
                ids[s] = x[s, R - 1, 0] = -11
                if R > 1:
                    x[s, 0, 0] = 11
            else:              # a NaN id matches nothing
                ids[s] = np.nan if nan else 5001
    return x, ids


def want_own(x, ids):
    """(mine_idx [n], own rows [n, 31]) by the rule of SPEC §21, in numpy."""
    idx = np.zeros(len(ids), dtype=np.int64)
    for m in range(len(ids)):
        hit = np.nonzero((x[m, :, 0] == ids[m]) & (x[m, :, 0] != 0))[0]
        idx[m] = hit[0] if len(hit) else 0
    return idx, x[np.arange(len(ids)), idx]


def mask_pattern(p, R, rng):
    """R + 1 legal bits: none, the no-op alone, all, the edges of every 64-entry block, sparse."""
    b = np.zeros(R + 1, dtype=bool)
    j = np.arange(R)
    if p == 1:
        b[R] = True
    elif p == 2:
        b[:] = True
    elif p == 3:
        b[:R] = (j == 0) | (j == R - 1) | (j % 64 == 63) | (j % 64 == 0)
    elif p == 4:
        b[:R] = rng.random(R) < max(0.01, 2.0 / R)
        b[R] = True
    return b


class Case:
    """N rows of H heads over sets of R candidates (row r reads set r // share), float32 in flat rows
    (`elem` 0) or int16."""

    def __init__(self, kind, n, R, elem, share=1):
        rng = np.random.default_rng(1000 * n + R + 7 * share + kind.code)
        self.kind, self.n, self.R, self.elem, self.share = kind, n, R, elem, share
        self.H = H = (ENTITY_HEADS if kind is ENTITY else ITEM_HEADS)[R]
        self.m = m = -(-n // share)
        W, cols = R + 1, kind.cols
        f32 = elem == F32
        sets, ids = make_sets(kind, m, R, rng, nan=f32)
        if m * R >= 64:  # every edge value is there
            for col, vals in EDGES[kind.name].items():
                assert set(vals) <= set(sets[:, :, col].reshape(-1).tolist()), (kind.name, n, R, col)
        legal = np.stack([[mask_pattern((r + h) % 5, R, rng) for h in range(H)] for r in range(n)])  # [n, H, W]
        if n == 1 and R == 100:
            legal[0, :] = [mask_pattern(p, R, rng) for p in (3, 0, 4)]
        self.legal = torch.from_numpy(legal).to(DEV)
        self.sets = torch.from_numpy(sets).to(DEV)  # [m, R, cols] float32, exact for int16 too
        self.set_of = torch.arange(n, device=DEV) // share
        if kind is ENTITY:
            self.want_idx, own = want_own(sets, ids)
            self.want_mine = torch.from_numpy(own).to(DEV)  # [n, 31] raw columns of the own row
        # what the logits kernels read: candidates illegal in every head of every row that reads their set are NaN
        used = np.zeros((m, R), dtype=bool)
        np.logical_or.at(used, np.arange(n) // share, legal[:, :, :R].any(1))
        poisoned = sets.copy()
        if f32:
            poisoned[~used] = np.nan
        self.mask_off = [3 + h * W for h in range(H)]
        assert 3 + H * W < ID_OFF and OFF + cols * R < ROW
        if f32:
            buf = torch.from_numpy(rng.integers(-9, 9, (n, ROW)).astype(np.float32))
            buf[:m, OFF:OFF + cols * R] = torch.from_numpy(sets.reshape(m, -1))
            buf[:m, ID_OFF] = torch.from_numpy(ids)
            vals = np.where(legal, rng.choice([1.0, 0.5, 3.0], legal.shape), rng.choice([0.0, -1.0], legal.shape))
            buf[:, 3:3 + H * W] = torch.from_numpy(vals.reshape(n, -1).astype(np.float32))
            self.buf = buf.to(DEV)
            self.mask = self.buf
            self.ents = self.buf[:m, OFF:OFF + cols * R]
            self.ids = self.buf[:m, ID_OFF]
            self.pbuf = self.buf.clone()
            self.pbuf[:m, OFF:OFF + cols * R] = torch.from_numpy(poisoned.reshape(m, -1)).to(DEV)
            self.pmask = self.pbuf
            self.pents = self.pbuf[:m, OFF:OFF + cols * R]
        else:
            stride = (cols * R + 38) | 1  # odd: rows are 2-byte aligned only
            buf = torch.from_numpy(rng.integers(-9, 9, (m, stride)).astype(np.int16))
            buf[:, 5:5 + cols * R] = torch.from_numpy(sets.reshape(m, -1).astype(np.int16))
            buf[:, 2] = torch.from_numpy(ids.astype(np.int16))
            self.buf = buf.to(DEV)
            self.ents = self.buf[:, 5:5 + cols * R]
            self.ids = self.buf[:, 2]
            self.mask = torch.zeros((n, 3 + H * W + 2), dtype=torch.uint8, device=DEV)
            self.mask[:, 3:3 + H * W] = self.legal.reshape(n, -1).to(torch.uint8) * 3
            self.pbuf, self.pmask, self.pents = self.buf, self.mask, self.ents  # int16 has no NaN
        self.pq = torch.from_numpy(rng.standard_normal((n, H, kind.query)).astype(np.float32)).to(DEV)
        self.out_off = [1 + h * (W + 1) for h in range(H)]  # a canary entry between the heads
        self.out_stride = 1 + H * (W + 1) + 4
        self.keep, self.pkeep = self.buf.clone(), self.pbuf.clone()

    def unchanged(self):
        def bits(t):
            return t.view(torch.int32) if t.dtype == torch.float32 else t
        return torch.equal(bits(self.buf), bits(self.keep)) and torch.equal(bits(self.pbuf), bits(self.pkeep))

    def raw(self, fn, last, last_stride, other):
        x, stride, rows, ek = _sets.set_arg(self.pents, None, self.kind.spec)
        assert (rows, ek) == (self.R, self.elem) and x.data_ptr() == self.pents.data_ptr()
        sh = _sets.set_heads_struct(self.mask_off, self.out_off, self.kind.name)
        _, mptr, mstride, mkind = heads._mask_arg(self.pmask, self.n, self.mask_off[-1] + self.R + 1)
        assert mptr == self.pmask.data_ptr()
        args = [self.kind.code, ctypes.byref(sh), self.n, x.data_ptr(), stride, ek, rows, self.share, mptr, mstride, mkind]
        args += [other.data_ptr(), last.data_ptr(), last_stride] if fn == "nmh_embed_logits" else \
            [last.data_ptr(), last_stride, other.data_ptr()]
        heads.check(getattr(heads.lib(), fn)(*args, heads._stream()), fn)
        torch.cuda.synchronize()

    def logits(self):
        out = torch.full((self.n, self.out_stride), CANARY, dtype=torch.float32, device=DEV)
        self.raw("nmh_embed_logits", out, self.out_stride, self.pq)
        return out

    def backward(self, g_out):
        g_pq = torch.full((self.n, self.H, self.kind.query), CANARY, dtype=torch.float32, device=DEV)
        self.raw("nmh_embed_logits_backward", g_out, self.out_stride, g_pq)
        return g_pq

    def row_features64(self):
        """X [n, R, Q] float64 of the rows' (unpoisoned) sets, in pq's layout: the D one-hots of 256,
        the C scaled columns, 1 for the bias and zero pads, so that a logit is pq . X."""
        k = self.kind
        idx, cont = embed.embed_features_ref(k, self.sets.double())
        hot = torch.nn.functional.one_hot(idx, embed.BINS).double().flatten(-2)
        x = torch.cat([hot, cont, cont.new_ones(*cont.shape[:-1], 1), cont.new_zeros(*cont.shape[:-1], k.query - k.bias - 1)], -1)
        return x[self.set_of]

    def head_slices(self, t):
        """[n, H, R + 1] of an out / g_out shaped tensor."""
        return torch.stack([t[:, o:o + self.R + 1] for o in self.out_off], 1)


_cases = {}


def case(kind, n, R, elem, share=1):
    key = (kind.name, n, R, elem, share)
    if key not in _cases:
        _cases[key] = Case(kind, n, R, elem, share)
    return _cases[key]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def check_features_counts_and_sums(kind, ents, sets):
    """ents: what the kernels read in place; sets: the same values, [M, R, cols] float32."""
    want_idx, want_cont = embed.embed_features_ref(kind, sets)
    idx, cont = embed.embed_features(kind, ents)
    assert idx.dtype == torch.uint8 and torch.equal(idx.long(), want_idx)
    assert cont.dtype == torch.float32 and same_bits(cont, want_cont)
    (c1, s1), (c2, s2) = embed.embed_counts(kind, ents), embed.embed_counts(kind, ents)
    assert same_bits(c1, c2) and same_bits(s1, s2)
    assert torch.equal(c1, torch.nn.functional.one_hot(want_idx, embed.BINS).sum(1).float())
    assert torch.equal(c1.sum(-1), torch.full_like(c1[..., 0], sets.shape[1]))
    raw = sets[..., list(kind.ccols)].double().sum(1)
    assert float(raw.abs().max()) < 2 ** 24
    assert torch.equal(s1.double(), raw), (s1.double() - raw).abs().max()
    return idx, cont, c1, s1


def check_own(c):
    want_i, want_c = embed.embed_features_ref(ENTITY, c.want_mine)
    mine_i, mine_c, idx = embed.embed_own(c.ents, c.ids)
    assert idx.dtype == torch.int32 and idx.cpu().tolist() == c.want_idx.tolist(), (idx, c.want_idx)
    assert mine_i.dtype == torch.uint8 and torch.equal(mine_i.long(), want_i) and same_bits(mine_c, want_c)
    assert torch.equal(embed.own_row_ref(c.sets, c.ids).cpu(), torch.from_numpy(c.want_idx))
    return mine_i, mine_c, idx


def check_logits(c):
    k = c.kind
    out = c.logits()
    assert c.unchanged()
    got = c.head_slices(out)  # [n, H, R + 1]
    canary = torch.ones_like(out, dtype=torch.bool)
    for o in c.out_off:
        canary[:, o:o + c.R + 1] = False
    assert bool((out[canary] == CANARY).all()), "a store outside the heads' entries"
    assert bool(torch.isfinite(got).all()), "a NaN of a candidate that no head allows"
    legal = c.legal.clone()
    legal[:, :, c.R] = False  # the no-op entry is 0 whatever its mask says
    assert bool((got[~legal].view(torch.int32) == 0).all()), "illegal and no-op entries are +0.0f"
    x = c.row_features64()  # [n, R, Q]
    pq = c.pq.double()
    want = torch.einsum("nhf,njf->nhj", pq, x)
    bound = (k.D + 2 * k.C + 1) * EPS * torch.einsum("nhf,njf->nhj", pq.abs(), x.abs())
    err = (got[..., :c.R].double() - want).abs()
    sel = legal[..., :c.R]
    print(f"logits {k.name} n={c.n} R={c.R} elem={c.elem} share={c.share}: legal {int(sel.sum())}, max err/bound "
          f"{float((err / bound.clamp_min(1e-300))[sel].max()) if sel.any() else 0:.3f}")
    assert bool(((err <= bound) | ~sel).all())
    return got


def check_backward(c):
    k = c.kind
    legal = c.legal.clone()
    legal[:, :, c.R] = False
    g = torch.randn((c.n, c.H, c.R + 1), device=DEV) * 2
    g_out = torch.full((c.n, c.out_stride), float("nan"), dtype=torch.float32, device=DEV)
    for h, o in enumerate(c.out_off):  # NaN wherever the kernel has no business reading
        g_out[:, o:o + c.R + 1] = torch.where(legal[:, h], g[:, h], torch.full_like(g[:, h], float("nan")))
    g1, g2 = c.backward(g_out), c.backward(g_out)
    assert c.unchanged()
    assert same_bits(g1, g2)
    assert bool((g1[..., k.bias + 1:].view(torch.int32) == 0).all()), "the pads are 0"
    # float64 autograd through the materialised features
    x = c.row_features64()
    pq = c.pq.double().clone().requires_grad_(True)
    lg = torch.einsum("nhf,njf->nhj", pq, x)
    g64 = torch.where(legal[..., :c.R], g[..., :c.R].double(), torch.zeros((), dtype=torch.float64, device=DEV))
    (want,) = torch.autograd.grad((lg * g64).sum(), pq)
    cnt = legal.sum(-1, keepdim=True).double()
    bound = (cnt + 1) * EPS * torch.einsum("nhj,njf->nhf", g64.abs(), x.abs())
    err = (g1.double() - want).abs()
    assert bool(torch.isfinite(g1).all()), "a NaN of g_out or of a candidate that no head allows"
    print(f"backward {k.name} n={c.n} R={c.R} elem={c.elem} share={c.share}: max err/bound "
          f"{float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    return g1


ELEMS = [F32, I16]


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("n,R", ENTITY_SHAPES)
def test_entity_features_counts_sums_and_own_row(n, R, elem):
    c = case(ENTITY, n, R, elem)
    idx, cont, counts, sums = check_features_counts_and_sums(ENTITY, c.ents, c.sets)
    mine_i, mine_c, mine_idx = check_own(c)
    assert c.unchanged()
    # the same sets as a [N, R, 31] tensor, and ids as [N, 1]
    dense = c.sets if elem == F32 else c.sets.to(torch.int16)
    i2, c2 = embed.embed_features(ENTITY, dense)
    assert torch.equal(i2, idx) and same_bits(c2, cont)
    m2 = embed.embed_own(dense, c.ids.reshape(-1, 1))
    assert torch.equal(m2[0], mine_i) and same_bits(m2[1], mine_c) and torch.equal(m2[2], mine_idx)
    # all seven outputs of one call
    out = embed._call(ENTITY, c.ents, c.ids, None, ("idx", "cont", "counts", "sums", "mine_idx", "mine_i", "mine_c"))
    torch.cuda.synchronize()
    assert torch.equal(out["idx"], idx) and same_bits(out["cont"], cont) and same_bits(out["counts"], counts)
    assert same_bits(out["sums"], sums) and torch.equal(out["mine_idx"], mine_idx)
    assert torch.equal(out["mine_i"], mine_i) and same_bits(out["mine_c"], mine_c) and c.unchanged()


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("n,R,share", ITEM_SHAPES)
def test_item_features_counts_and_sums(n, R, share, elem):
    c = case(ITEM, n, R, elem, share)
    check_features_counts_and_sums(ITEM, c.ents, c.sets)
    assert c.unchanged()


def test_the_item_kind_has_no_own_row():
    z = torch.zeros((2, 4, 16), device=DEV)
    with pytest.raises(heads.HeadsError, match="are the entity kind's"):
        embed._call(ITEM, z, torch.zeros(2, device=DEV), None, ("mine_idx",))


@pytest.mark.parametrize("kind,R", [(ENTITY, 1), (ENTITY, 100), (ENTITY, 256), (ITEM, 12), (ITEM, 1024)])
def test_all_zero_sets(kind, R):
    z = torch.zeros((3, R, kind.cols), device=DEV)
    idx, cont = embed.embed_features(kind, z)
    want = torch.tensor([min(255, int(o)) for o in kind.doffs], dtype=torch.uint8, device=DEV)
    assert torch.equal(idx, want.expand(3, R, kind.D)) and not bool(cont.any())
    counts, sums = embed.embed_counts(kind, z.to(torch.int16))
    assert not bool(sums.any()) and torch.equal(counts.sum(-1), torch.full((3, kind.D), float(R), device=DEV))
    assert all(float(counts[0, d, int(want[d])]) == R for d in range(kind.D))
    if kind is ENTITY:
        mine_i, mine_c, mine_idx = embed.embed_own(z, torch.zeros(3, device=DEV))
        assert torch.equal(mine_i, want.expand(3, kind.D)) and not bool(mine_c.any()) and mine_idx.tolist() == [0, 0, 0]


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("n,R", ENTITY_SHAPES)
def test_entity_logits(n, R, elem):
    check_logits(case(ENTITY, n, R, elem))


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("n,R,share", ITEM_SHAPES)
def test_item_logits(n, R, share, elem):
    check_logits(case(ITEM, n, R, elem, share))


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("n,R", ENTITY_SHAPES)
def test_entity_logits_backward(n, R, elem):
    check_backward(case(ENTITY, n, R, elem))


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("n,R,share", ITEM_SHAPES)
def test_item_logits_backward(n, R, share, elem):
    check_backward(case(ITEM, n, R, elem, share))


@pytest.mark.parametrize("kind,n,R,elem,share", [(ENTITY, 9, 100, F32, 1), (ITEM, 9, 1024, I16, 3)])
def test_autograd_function_returns_the_kernels_gradient_to_the_table(kind, n, R, elem, share):
    c = case(kind, n, R, elem, share)
    enc = (embed.ReducedPlayerEncoder if kind is ENTITY else embed.ReducedItemEncoder)(64, 64, fused=True).to(DEV)
    q = torch.randn((n, c.H, 64), device=DEV, requires_grad=True)
    pq = enc.pointer_query(q)
    pq.retain_grad()
    out = embed.embed_logits(kind, c.pents, pq, c.pmask, c.mask_off, share=share)
    assert out.shape == (n, c.H * (R + 1))
    legal = c.legal.clone()
    legal[:, :, R] = False
    g = torch.where(legal.reshape(n, -1), torch.randn_like(out), torch.zeros_like(out))
    out.backward(g)
    g_out = torch.full((n, c.out_stride), float("nan"), dtype=torch.float32, device=DEV)
    for h, o in enumerate(c.out_off):
        g_out[:, o:o + R + 1] = g[:, h * (R + 1):(h + 1) * (R + 1)]
    keep, c.pq = c.pq, pq.detach()
    try:
        assert same_bits(c.head_slices(c.logits()), out.detach().reshape(n, c.H, R + 1))
        assert same_bits(c.backward(g_out), pq.grad)
    finally:
        c.pq = keep
    assert pq.grad.abs().sum() > 0
    layer = enc.agent_fc if kind is ENTITY else enc.fc
    for t in (q.grad, layer.weight.grad, layer.bias.grad, enc.embedding.weight.grad):
        assert t is not None and bool(torch.isfinite(t).all()) and t.abs().sum() > 0
    assert not bool(enc.embedding.weight.grad[embed.BINS:].any())  # the clip comes after the offset
    # the fused encoder's features and pool against the unfused one's
    twin = type(enc)(64, 64).to(DEV)
    twin.load_state_dict(enc.state_dict())
    exact = type(enc)(64, 64).to(DEV)
    exact.load_state_dict(enc.state_dict())
    exact = exact.double()
    with torch.no_grad():
        assert torch.equal(enc.features(c.ents), twin.features(c.sets))
        within(f"{kind.name} pooled", enc.pooled(c.ents).cpu().numpy(), exact.pooled(c.sets.double()).cpu().numpy(),
               twin.pooled(c.sets).double().cpu().numpy())


def test_a_fused_market_pass_and_buy_head_stay_below_the_embeddings_bytes():
    N, H, R = 64, 64, 1024
    rng = np.random.default_rng(5)
    items = torch.from_numpy(make_sets(ITEM, N, R, rng, nan=False)[0]).to(DEV)
    mask = torch.rand((N, R + 1), device=DEV) < 0.1
    q = torch.randn((N, 1, H), device=DEV)
    fused = embed.ReducedItemEncoder(H, H, fused=True).to(DEV)
    unfused = embed.ReducedItemEncoder(H, H).to(DEV)
    limit = N * R * H * 4

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.no_grad():
            fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    def fused_pass():
        fused.pooled(items)
        embed.embed_logits(ITEM, items, fused.pointer_query(q), mask, [0])

    rise_fused, rise_unfused = peak(fused_pass), peak(lambda: unfused.embed(items))
    print(f"peak rise: fused {rise_fused} B, unfused {rise_unfused} B, the embedding {limit} B")
    assert rise_fused < limit
    assert rise_unfused > limit
