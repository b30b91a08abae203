"""The player-encoder kernels (nmmo_amd/csrc/player_enc.hip, nmmo_amd/player.py, SPEC.md §21) on MI355X.

Inputs are synthetic Entity sections inside rows of 23,987 floats (so consecutive rows' sections lie
at 0 / 12 / 8 / 4 bytes modulo 16) and int16 sections at an odd offset of rows with an odd element
stride, for N in {1, 5, 9} rows (the last workgroup is partial) and R in {1, 63, 64, 65, 100, 256}
entities per set. Columns hold integers, +-32,767 among them, about half the entities are all zero,
npc_type takes 0..4, -3, 9 and (float32 only) NaN, and one set is all zero.

- features: bit-equal to `player_features_ref` on the GPU.
- sums: equal to the float64 sums (the columns hold integers with |sum| < 2^24, so the float32 sum is
  exact in any order; the class counts are exact), and identical on two runs.
- own row: `mine_idx` and `mine` exact on a match at entity 0, at entity R - 1, two matches (the
  first wins), no match, id 0 among zero-id entities, a negative NPC id and (float32 ids) a NaN id;
  alone and in one call with the features and the sums.
- logits: illegal and no-op entries exactly 0.0f. A legal entry is within 32 * 2^-24 * sum|terms| of
  float64, the bound per entry from the float64 terms. SPEC §21 fixes the order: one addition,
  pq[35] + pq[1 + t], then 30 fused multiply-adds (column 0 and columns 2..30), each of the 31
  operations rounding once and the features themselves being exact: 31 roundings, each at most
  2^-24 of a partial sum that sum|terms| bounds to first order, and one more for the second-order
  terms: (31 + 1) * 2^-24. The entities illegal in every head of the call are NaN in every column
  and the outputs must be finite. A canary around every head's R + 1 entries stays untouched and the
  buffer is unchanged bitwise.
- logits_backward: within (cnt + 1) * 2^-24 * sum|terms| of float64 autograd through the
  materialised features (cnt fused multiply-adds over the head's cnt legal candidates, the features
  exact); pads 0; illegal and no-op entries of g_out are NaN and must not leak; identical on two runs.
"""

import ctypes

import numpy as np
import pytest
import torch

from nmmo_amd import heads, player
from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

ROW = 23987  # floats of a flat obs row: rows' sections at 0 / 12 / 8 / 4 bytes mod 16
OFF = 1111   # the Entity section of a synthetic row; the float masks of up to 4 heads lie in front
ID_OFF = 1101  # the row's AgentId element
HEADS = {1: 4, 63: 3, 64: 4, 65: 3, 100: 3, 256: 4}
SHAPES = [(1, 1), (5, 63), (9, 64), (5, 65), (9, 100), (1, 100), (5, 256)]
EPS = 2.0 ** -24
ROUNDINGS = 31  # one addition and 30 fused multiply-adds (SPEC §21)
CANARY = 7.5
DEV = "cuda"
OWN_CASES = 7  # set m's own-row case is m % 7


def make_sets(n, R, rng, nan=True):
    """[n, R, 31] float32 integer-valued entity sets and the rows' ids [n]: about half the entities
    all zero, distinct ids (NPCs negative), the classes the clamp is for, +-32,767 columns, the
    middle set all zero; set m's id is placed for own-row case m % 7 (see `want_own`)."""
    x = rng.integers(-300, 3000, (n, R, 31)).astype(np.float32)
    ident = np.stack([rng.permutation(np.arange(1000, 1000 + R)) for _ in range(n)]).astype(np.float32)
    x[:, :, 0] = np.where(rng.random((n, R)) < 0.3, -ident, ident)
    x[:, :, 1] = rng.integers(0, 5, (n, R))
    x[rng.random((n, R)) < 0.5] = 0
    flat = x.reshape(n * R, 31)
    k = flat.shape[0]
    for i, t in enumerate([0, 4, -3, 9, np.nan if nan else 4, 2]):
        flat[(i * 7) % k, 1] = t
    flat[(3 * k) // 4, 2:30] = [32767, -32767] * 14
    flat[k // 3, 30] = -32767
    if n > 1:
        x[n // 2] = 0
    ids = np.zeros(n, dtype=np.float32)
    for m in range(n):
        case = m % OWN_CASES
        if case == 0:      # a match at entity 0
            ids[m] = x[m, 0, 0] = 7
        elif case == 1:    # a match at entity R - 1
            ids[m] = x[m, R - 1, 0] = 8
        elif case == 2:    # two matches: the first wins (one match when R < 3)
            ids[m] = x[m, R // 2, 0] = x[m, R - 1, 0] = 9
        elif case == 3:    # no match
            ids[m] = 5000
        elif case == 4:    # id 0 among zero-id entities
            ids[m] = 0
            x[m, R // 3, 0] = 0
        elif case == 5:    # a negative NPC id, its positive twin in front of it (when R > 1)
            ids[m] = x[m, R - 1, 0] = -11
            if R > 1:
                x[m, 0, 0] = 11
        else:              # a NaN id matches nothing
            ids[m] = np.nan if nan else 5001
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
    """N rows of H heads over sets of R entities, float32 in flat rows (`kind` 0) or int16."""

    def __init__(self, n, R, kind, seed=0):
        rng = np.random.default_rng(1000 * n + R + seed)
        self.n, self.R, self.H, self.kind = n, R, HEADS[R], kind
        H, W = self.H, R + 1
        f32 = kind == player.PLAYER_F32
        sets, ids = make_sets(n, R, rng, nan=f32)
        legal = np.stack([[mask_pattern((r + h) % 5, R, rng) for h in range(H)] for r in range(n)])  # [n, H, W]
        if n == 1 and R == 100:
            legal[0, :] = [mask_pattern(p, R, rng) for p in (3, 0, 4)]
        self.legal = torch.from_numpy(legal).to(DEV)
        self.want_idx, own = want_own(sets, ids)
        self.want_mine = torch.from_numpy(own).to(DEV)  # [n, 31] raw columns of the own row
        self.sets = torch.from_numpy(sets).to(DEV)  # [n, R, 31] float32, exact for int16 too
        # what the logits kernels read: the entities illegal in every head are NaN in every column
        poisoned = sets.copy()
        if f32:
            poisoned[~legal[:, :, :R].any(1)] = np.nan
        self.mask_off = [3 + h * W for h in range(H)]
        if f32:
            buf = torch.from_numpy(rng.integers(-9, 9, (n, ROW)).astype(np.float32))
            buf[:, OFF:OFF + 31 * R] = torch.from_numpy(sets.reshape(n, -1))
            buf[:, ID_OFF] = torch.from_numpy(ids)
            vals = np.where(legal, rng.choice([1.0, 0.5, 3.0], legal.shape), rng.choice([0.0, -1.0], legal.shape))
            buf[:, 3:3 + H * W] = torch.from_numpy(vals.reshape(n, -1).astype(np.float32))
            self.buf = buf.to(DEV)
            self.mask = self.buf
            self.ents = self.buf[:, OFF:OFF + 31 * R]
            self.ids = self.buf[:, ID_OFF]
            self.pbuf = self.buf.clone()
            self.pbuf[:, OFF:OFF + 31 * R] = torch.from_numpy(poisoned.reshape(n, -1)).to(DEV)
            self.pmask = self.pbuf
            self.pents = self.pbuf[:, OFF:OFF + 31 * R]
        else:
            stride = (31 * R + 38) | 1  # odd: rows are 2-byte aligned only
            buf = torch.from_numpy(rng.integers(-9, 9, (n, stride)).astype(np.int16))
            buf[:, 5:5 + 31 * R] = torch.from_numpy(sets.reshape(n, -1).astype(np.int16))
            buf[:, 2] = torch.from_numpy(ids.astype(np.int16))
            self.buf = buf.to(DEV)
            self.ents = self.buf[:, 5:5 + 31 * R]
            self.ids = self.buf[:, 2]
            self.mask = torch.zeros((n, 3 + H * W + 2), dtype=torch.uint8, device=DEV)
            self.mask[:, 3:3 + H * W] = self.legal.reshape(n, -1).to(torch.uint8) * 3
            self.pbuf, self.pmask, self.pents = self.buf, self.mask, self.ents  # int16 has no NaN
        self.pq = torch.from_numpy(rng.standard_normal((n, H, 40)).astype(np.float32)).to(DEV)
        self.out_off = [1 + h * (W + 1) for h in range(H)]  # a canary entry between the heads
        self.out_stride = 1 + H * (W + 1) + 4
        self.keep, self.pkeep = self.buf.clone(), self.pbuf.clone()

    def unchanged(self):
        def bits(t):
            return t.view(torch.int32) if t.dtype == torch.float32 else t
        return torch.equal(bits(self.buf), bits(self.keep)) and torch.equal(bits(self.pbuf), bits(self.pkeep))

    def raw(self, fn, last, last_stride, other):
        x, stride, rows, kind = player._ent_arg(self.pents, None)
        assert (rows, kind) == (self.R, self.kind) and x.data_ptr() == self.pents.data_ptr()
        ph = player.player_heads_struct(self.mask_off, self.out_off)
        _, mptr, mstride, mkind = heads._mask_arg(self.pmask, self.n, self.mask_off[-1] + self.R + 1)
        assert mptr == self.pmask.data_ptr()
        args = [ctypes.byref(ph), self.n, x.data_ptr(), stride, kind, rows, mptr, mstride, mkind]
        args += [other.data_ptr(), last.data_ptr(), last_stride] if fn == "nmh_player_logits" else \
            [last.data_ptr(), last_stride, other.data_ptr()]
        heads.check(getattr(heads.lib(), fn)(*args, heads._stream()), fn)
        torch.cuda.synchronize()

    def logits(self):
        out = torch.full((self.n, self.out_stride), CANARY, dtype=torch.float32, device=DEV)
        self.raw("nmh_player_logits", out, self.out_stride, self.pq)
        return out

    def backward(self, g_out):
        g_pq = torch.full((self.n, self.H, 40), CANARY, dtype=torch.float32, device=DEV)
        self.raw("nmh_player_logits_backward", g_out, self.out_stride, g_pq)
        return g_pq

    def row_features64(self):
        """x~ = (x, 1) [n, R, 36] float64 (of the unpoisoned sets)."""
        x = player.player_features_ref(self.sets.double())
        return torch.cat([x, x.new_ones(self.n, self.R, 1)], -1)

    def head_slices(self, t):
        """[n, H, R + 1] of an out / g_out shaped tensor."""
        return torch.stack([t[:, o:o + self.R + 1] for o in self.out_off], 1)


_cases = {}


def case(n, R, kind, **kw):
    key = (n, R, kind, tuple(sorted(kw.items())))
    if key not in _cases:
        _cases[key] = Case(n, R, kind, **kw)
    return _cases[key]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def check_features_and_sums(ents, sets):
    """ents: what the kernels read in place; sets: the same values, [N, R, 31] float32."""
    want = player.player_features_ref(sets)
    got = player.player_features(ents)
    assert got.dtype == torch.float32 and same_bits(got, want)
    s1, s2 = player.player_sums(ents), player.player_sums(ents)
    assert same_bits(s1, s2)
    raw = want.double().sum(1)
    assert float(raw.abs().max()) < 2 ** 24
    assert torch.equal(s1.double(), raw), (s1.double() - raw).abs().max()
    assert torch.equal(s1[:, 1:6].sum(1), torch.full_like(s1[:, 0], sets.shape[1]))
    return got, s1


def check_own(c):
    want_x = player.player_features_ref(c.want_mine)
    mine, idx = player.player_own(c.ents, c.ids)
    assert idx.dtype == torch.int32 and idx.cpu().tolist() == c.want_idx.tolist(), (idx, c.want_idx)
    assert mine.dtype == torch.float32 and same_bits(mine, want_x)
    ref_mine, ref_idx = player.own_row_ref(c.sets, c.ids)
    assert torch.equal(ref_idx.cpu(), torch.from_numpy(c.want_idx)) and torch.equal(ref_mine, want_x)
    return mine, idx


def check_logits(c):
    out = c.logits()
    assert c.unchanged()
    got = c.head_slices(out)  # [n, H, R + 1]
    canary = torch.ones_like(out, dtype=torch.bool)
    for o in c.out_off:
        canary[:, o:o + c.R + 1] = False
    assert bool((out[canary] == CANARY).all()), "a store outside the heads' entries"
    assert bool(torch.isfinite(got).all()), "a NaN of an entity that no head allows"
    legal = c.legal.clone()
    legal[:, :, c.R] = False  # the no-op entry is 0 whatever its mask says
    assert bool((got[~legal].view(torch.int32) == 0).all()), "illegal and no-op entries are +0.0f"
    x = c.row_features64()  # [n, R, 36]
    pq = c.pq.double()[..., :36]
    want = torch.einsum("nhf,njf->nhj", pq, x)
    bound = (ROUNDINGS + 1) * EPS * torch.einsum("nhf,njf->nhj", pq.abs(), x.abs())
    err = (got[..., :c.R].double() - want).abs()
    ok = (err <= bound) | ~legal[..., :c.R]
    sel = legal[..., :c.R]
    print(f"logits n={c.n} R={c.R} kind={c.kind}: legal {int(sel.sum())}, max err/bound "
          f"{float((err / bound.clamp_min(1e-300))[sel].max()) if sel.any() else 0:.3f}")
    assert bool(ok.all())
    return got


def check_backward(c):
    legal = c.legal.clone()
    legal[:, :, c.R] = False
    g = torch.randn((c.n, c.H, c.R + 1), device=DEV) * 2
    g_out = torch.full((c.n, c.out_stride), float("nan"), dtype=torch.float32, device=DEV)
    for h, o in enumerate(c.out_off):  # NaN wherever the kernel has no business reading
        g_out[:, o:o + c.R + 1] = torch.where(legal[:, h], g[:, h], torch.full_like(g[:, h], float("nan")))
    g1, g2 = c.backward(g_out), c.backward(g_out)
    assert c.unchanged()
    assert same_bits(g1, g2)
    assert bool((g1[..., 36:].view(torch.int32) == 0).all()), "the pads are 0"
    # float64 autograd through the materialised features
    x = c.row_features64()
    pq = c.pq.double()[..., :36].clone().requires_grad_(True)
    lg = torch.einsum("nhf,njf->nhj", pq, x)
    g64 = torch.where(legal[..., :c.R], g[..., :c.R].double(), torch.zeros((), dtype=torch.float64, device=DEV))
    (want,) = torch.autograd.grad((lg * g64).sum(), pq)
    cnt = legal.sum(-1, keepdim=True).double()
    bound = (cnt + 1) * EPS * torch.einsum("nhj,njf->nhf", g64.abs(), x.abs())
    err = (g1[..., :36].double() - want).abs()
    assert bool(torch.isfinite(g1).all()), "a NaN of g_out or of an entity that no head allows"
    print(f"backward n={c.n} R={c.R} kind={c.kind}: max err/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    return g1


KINDS = [player.PLAYER_F32, player.PLAYER_I16]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,R", SHAPES)
def test_features_sums_and_own_row(n, R, kind):
    c = case(n, R, kind)
    feats, sums = check_features_and_sums(c.ents, c.sets)
    mine, idx = check_own(c)
    assert c.unchanged()
    # the same sets as a [N, R, 31] tensor, and ids as [N, 1]
    dense = c.sets if kind == player.PLAYER_F32 else c.sets.to(torch.int16)
    assert same_bits(player.player_features(dense), feats) and same_bits(player.player_sums(dense), sums)
    m2, i2 = player.player_own(dense, c.ids.reshape(-1, 1))
    assert same_bits(m2, mine) and torch.equal(i2, idx)
    # all four outputs of one call
    x, stride, rows, k = player._ent_arg(c.ents, None)
    idt, id_stride, id_kind = player._id_arg(c.ids, n)
    outs = [torch.full(s, CANARY, dtype=torch.float32, device=DEV) for s in ((n, R, 35), (n, 35), (n, 35))]
    oidx = torch.full((n,), -5, dtype=torch.int32, device=DEV)
    heads.check(heads.lib().nmh_player_features(n, x.data_ptr(), stride, k, rows, idt.data_ptr(), id_stride, id_kind,
                                                *(t.data_ptr() for t in outs), oidx.data_ptr(), heads._stream()),
                "nmh_player_features")
    torch.cuda.synchronize()
    assert same_bits(outs[0], feats) and same_bits(outs[1], sums) and same_bits(outs[2], mine)
    assert torch.equal(oidx, idx) and c.unchanged()


def test_an_id_of_the_other_kind():
    """float32 entities with int16 ids and int16 entities with float32 ids (a NaN among them)."""
    c = case(9, 100, player.PLAYER_F32)
    ids16 = torch.nan_to_num(c.ids, nan=5001.0).to(torch.int16)
    mine, idx = player.player_own(c.ents, ids16)
    w_idx, w_own = want_own(c.sets.cpu().numpy(), ids16.float().cpu().numpy())
    assert idx.cpu().tolist() == w_idx.tolist()
    assert same_bits(mine, player.player_features_ref(torch.from_numpy(w_own).to(DEV)))
    d = case(9, 100, player.PLAYER_I16)
    idf = d.ids.float()
    idf[6] = float("nan")
    mine, idx = player.player_own(d.ents, idf)
    w_idx, w_own = want_own(d.sets.cpu().numpy(), idf.cpu().numpy())
    assert idx.cpu().tolist() == w_idx.tolist() and w_idx[6] == 0
    assert same_bits(mine, player.player_features_ref(torch.from_numpy(w_own).to(DEV)))


@pytest.mark.parametrize("R", [1, 64, 100, 256])
def test_all_zero_sets(R):
    z = torch.zeros((3, R, 31), device=DEV)
    f, s = player.player_features(z), player.player_sums(z)
    want = torch.zeros(35, device=DEV)
    want[1] = 1
    assert torch.equal(f, want.expand(3, R, 35)) and torch.equal(s, (want * R).expand(3, 35))
    assert torch.equal(player.player_sums(z.to(torch.int16)), s)
    mine, idx = player.player_own(z, torch.zeros(3, device=DEV))
    assert torch.equal(mine, want.expand(3, 35)) and idx.tolist() == [0, 0, 0]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,R", SHAPES)
def test_logits(n, R, kind):
    check_logits(case(n, R, kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,R", SHAPES)
def test_logits_backward(n, R, kind):
    check_backward(case(n, R, kind))


@pytest.mark.parametrize("n,R,kind", [(9, 100, player.PLAYER_F32), (5, 256, player.PLAYER_I16)])
def test_autograd_function_returns_the_kernels_gradient_to_the_query(n, R, kind):
    c = case(n, R, kind)
    enc = player.PlayerEncoder(64, 64, fused=True).to(DEV)
    q = torch.randn((n, c.H, 64), device=DEV, requires_grad=True)
    pq = enc.pointer_query(q)
    pq.retain_grad()
    out = player.player_logits(c.pents, pq, c.pmask, c.mask_off)
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
    for t in (q.grad, enc.agent_fc.weight.grad, enc.agent_fc.bias.grad):
        assert t is not None and bool(torch.isfinite(t).all()) and t.abs().sum() > 0
    assert enc.my_agent_fc.weight.grad is None
