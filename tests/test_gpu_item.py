"""The item-encoder kernels (nmmo_amd/csrc/item_enc.hip, nmmo_amd/item.py, SPEC.md §20) on MI355X.

Inputs are synthetic item sections inside rows of 23,987 floats (so consecutive rows' sections lie at
0 / 12 / 8 / 4 bytes modulo 16) and int16 sections at an odd offset of rows with an odd element
stride, for N in {1, 5, 9} rows (the last workgroup is partial) and R in {1, 12, 63, 65, 257, 1024}
items per set; and the engine's own obs rows of a saturated state.

- features: bit-equal to `item_features_ref` on the GPU.
- sums: equal to the float64 sum rounded once (the columns hold integers with |sum| < 2^24, so the
  float32 sum is exact in any order) times 0.01f, and identical on two runs.
- logits: illegal and no-op entries exactly 0.0f; a legal entry within 16 * 2^-24 * sum|terms| of
  float64, the bound per entry from the float64 terms: the kernel rounds once per scaled feature and
  once per each of its 14 additions, each rounding at most 2^-24 of sum|terms|. A canary around every
  head's R + 1 entries stays untouched and the rows are unchanged.
- logits_backward: within (cnt + 16) * 2^-24 * sum|terms| of float64 autograd through the
  materialised features (cnt fused multiply-adds and one rounding of the feature per term); pads 0;
  illegal and no-op entries of g_out are NaN and must not be read; identical on two runs.
"""

import ctypes

import numpy as np
import pytest
import torch

from nmmo_amd import heads, item, layout
from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

ROW = 23987  # floats of a flat obs row: rows' sections at 0 / 12 / 8 / 4 bytes mod 16
OFF = 4108   # the item section of a synthetic row; the float masks of up to 4 heads lie in front
HEADS = {1: 4, 12: 4, 63: 3, 65: 4, 257: 2, 1024: 4}
SHAPES = [(1, 1), (5, 12), (9, 63), (5, 65), (9, 257), (5, 1024), (1, 1024)]
EPS = 2.0 ** -24
CANARY = 7.5
DEV = "cuda"


def make_sets(m, R, rng, nan=True):
    """[m, R, 16] float32 integer-valued item sets: about half the slots empty, every type, the
    classes the clamps are for, negative and +-32,767 columns; the middle set all zero."""
    x = rng.integers(-300, 3000, (m, R, 16)).astype(np.float32)
    x[:, :, 1] = rng.integers(0, 18, (m, R))
    x[:, :, 14] = rng.integers(0, 2, (m, R))
    x[rng.random((m, R)) < 0.5] = 0
    flat = x.reshape(m * R, 16)
    k = flat.shape[0]
    for i, (t, e) in enumerate([(0, 0), (17, 1), (-3, 5), (40, 0), (np.nan if nan else 17, 1), (5, 5)]):
        flat[(i * 7) % k, 1], flat[(i * 7) % k, 14] = t, e
    flat[(3 * k) // 4, 2:14] = [32767, -32767] * 6
    flat[k // 3, 15] = -32767
    if m > 1:
        x[m // 2] = 0
    return x


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
    """N rows of H heads over sets of R items, float32 in flat rows (`kind` 0) or int16."""

    def __init__(self, n, R, kind, seed=0, share=1):
        rng = np.random.default_rng(1000 * n + R + seed)
        self.n, self.R, self.H, self.kind, self.share = n, R, HEADS[R], kind, share
        H, W = self.H, R + 1
        m = -(-n // share)
        sets = make_sets(m, R, rng, nan=kind == item.ITEM_F32)
        legal = np.stack([[mask_pattern((r + h) % 5, R, rng) for h in range(H)] for r in range(n)])  # [n, H, W]
        if n == 1 and R == 1024:
            legal[0, :] = [mask_pattern(p, R, rng) for p in (3, 2, 0, 4)]
        self.legal = torch.from_numpy(legal).to(DEV)
        if kind == item.ITEM_F32:
            buf = torch.from_numpy(rng.integers(-9, 9, (m if share > 1 else n, ROW)).astype(np.float32))
            buf[:, OFF:OFF + 16 * R] = torch.from_numpy(sets.reshape(m, -1))
            self.mask_off = [3 + h * W for h in range(H)]
            if share == 1:  # the masks in the rows' prefix: legal iff > 0
                vals = np.where(legal, rng.choice([1.0, 0.5, 3.0], legal.shape), rng.choice([0.0, -1.0], legal.shape))
                buf[:, 3:3 + H * W] = torch.from_numpy(vals.reshape(n, -1).astype(np.float32))
                self.buf = buf.to(DEV)
                self.mask = self.buf
            else:
                self.buf = buf.to(DEV)
                self.mask = torch.zeros((n, 3 + H * W), dtype=torch.float32, device=DEV)
                self.mask[:, 3:] = self.legal.reshape(n, -1).float()
            self.items = self.buf[:, OFF:OFF + 16 * R]
        else:
            stride = 16 * R + 37  # odd: rows are 2-byte aligned only
            buf = torch.from_numpy(rng.integers(-9, 9, (m, stride)).astype(np.int16))
            buf[:, 5:5 + 16 * R] = torch.from_numpy(sets.reshape(m, -1).astype(np.int16))
            self.buf = buf.to(DEV)
            self.items = self.buf[:, 5:5 + 16 * R]
            self.mask_off = [3 + h * W for h in range(H)]
            self.mask = torch.zeros((n, 3 + H * W + 2), dtype=torch.uint8, device=DEV)
            self.mask[:, 3:3 + H * W] = self.legal.reshape(n, -1).to(torch.uint8) * 3
        self.sets = torch.from_numpy(sets).to(DEV)  # [m, R, 16] float32, exact for int16 too
        self.pq = torch.from_numpy(rng.standard_normal((n, H, 36)).astype(np.float32)).to(DEV)
        self.out_off = [1 + h * (W + 1) for h in range(H)]  # a canary entry between the heads
        self.out_stride = 1 + H * (W + 1) + 4
        self.keep = self.buf.clone()

    def unchanged(self):
        a, b = (t.view(torch.int32) if t.dtype == torch.float32 else t for t in (self.buf, self.keep))
        return torch.equal(a, b)

    def raw(self, fn, last, last_stride, other):
        x, stride, rows, kind = item._item_arg(self.items, None)
        assert (rows, kind) == (self.R, self.kind) and x.data_ptr() == self.items.data_ptr()
        ih = item.item_heads_struct(self.mask_off, self.out_off)
        _, mptr, mstride, mkind = heads._mask_arg(self.mask, self.n, self.mask_off[-1] + self.R + 1)
        assert mptr == self.mask.data_ptr()
        args = [ctypes.byref(ih), self.n, x.data_ptr(), stride, kind, rows, self.share, mptr, mstride, mkind]
        args += [other.data_ptr(), last.data_ptr(), last_stride] if fn == "nmh_item_logits" else \
            [last.data_ptr(), last_stride, other.data_ptr()]
        heads.check(getattr(heads.lib(), fn)(*args, heads._stream()), fn)
        torch.cuda.synchronize()

    def logits(self):
        out = torch.full((self.n, self.out_stride), CANARY, dtype=torch.float32, device=DEV)
        self.raw("nmh_item_logits", out, self.out_stride, self.pq)
        return out

    def backward(self, g_out):
        g_pq = torch.full((self.n, self.H, 36), CANARY, dtype=torch.float32, device=DEV)
        self.raw("nmh_item_logits_backward", g_out, self.out_stride, g_pq)
        return g_pq

    def row_features64(self):
        """x~ = (x, 1) [n, R, 33] float64 of the set each row reads."""
        x = item.item_features_ref(self.sets.double()).repeat_interleave(self.share, 0)[:self.n]
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


def check_features_and_sums(items, sets):
    """items: what the kernels read in place; sets: the same values, [M, R, 16] float32."""
    want = item.item_features_ref(sets)
    got = item.item_features(items)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    s1, s2 = item.item_sums(items), item.item_sums(items)
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    raw = torch.nan_to_num(sets.double(), nan=0.0)[..., item.CONT_COLS].sum(1)
    assert float(raw.abs().max()) < 2 ** 24
    want_s = torch.cat([want[..., :20].double().sum(1).float(),
                        raw.float() * torch.tensor(0.01, dtype=torch.float32, device=raw.device)], 1)
    assert torch.equal(s1, want_s), (s1 - want_s).abs().max()


def check_logits(c):
    out = c.logits()
    assert c.unchanged()
    got = c.head_slices(out)  # [n, H, R + 1]
    canary = torch.ones_like(out, dtype=torch.bool)
    for o in c.out_off:
        canary[:, o:o + c.R + 1] = False
    assert bool((out[canary] == CANARY).all()), "a store outside the heads' entries"
    legal = c.legal.clone()
    legal[:, :, c.R] = False  # the no-op entry is 0 whatever its mask says
    assert bool((got[~legal].view(torch.int32) == 0).all()), "illegal and no-op entries are +0.0f"
    x = c.row_features64()  # [n, R, 33]
    pq = c.pq.double()[..., :33]
    want = torch.einsum("nhf,njf->nhj", pq, x)
    bound = 16 * EPS * torch.einsum("nhf,njf->nhj", pq.abs(), x.abs())
    err = (got[..., :c.R].double() - want).abs()
    ok = (err <= bound) | ~legal[..., :c.R]
    print(f"logits n={c.n} R={c.R} kind={c.kind}: legal {int(legal.sum())}, max err/bound "
          f"{float((err / bound.clamp_min(1e-300))[legal[..., :c.R]].max()) if legal.any() else 0:.3f}")
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
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32))
    assert bool((g1[..., 33:].view(torch.int32) == 0).all()), "the pads are 0"
    # float64 autograd through the materialised features
    x = c.row_features64()
    pq = c.pq.double()[..., :33].clone().requires_grad_(True)
    lg = torch.einsum("nhf,njf->nhj", pq, x)
    g64 = torch.where(legal[..., :c.R], g[..., :c.R].double(), torch.zeros((), dtype=torch.float64, device=DEV))
    (want,) = torch.autograd.grad((lg * g64).sum(), pq)
    cnt = legal.sum(-1, keepdim=True).double()
    bound = (cnt + 16) * EPS * torch.einsum("nhj,njf->nhf", g64.abs(), x.abs())
    err = (g1[..., :33].double() - want).abs()
    print(f"backward n={c.n} R={c.R} kind={c.kind}: max err/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    return g1


@pytest.mark.parametrize("kind", [item.ITEM_F32, item.ITEM_I16])
@pytest.mark.parametrize("n,R", SHAPES)
def test_features_and_sums(n, R, kind):
    c = case(n, R, kind)
    check_features_and_sums(c.items, c.sets)
    assert c.unchanged()
    # the same sets as a [M, R, 16] tensor
    dense = c.sets if kind == item.ITEM_F32 else c.sets.to(torch.int16)
    assert torch.equal(item.item_features(dense), item.item_features(c.items))
    assert torch.equal(item.item_sums(dense), item.item_sums(c.items))


@pytest.mark.parametrize("R", [1, 12, 65, 1024])
def test_all_zero_sets(R):
    z = torch.zeros((3, R, 16), device=DEV)
    f, s = item.item_features(z), item.item_sums(z)
    want = torch.zeros(32, device=DEV)
    want[0] = want[18] = 1
    assert torch.equal(f, want.expand(3, R, 32)) and torch.equal(s, (want * R).expand(3, 32))
    assert torch.equal(item.item_sums(z.to(torch.int16)), s)


@pytest.mark.parametrize("kind", [item.ITEM_F32, item.ITEM_I16])
@pytest.mark.parametrize("n,R", SHAPES)
def test_logits(n, R, kind):
    check_logits(case(n, R, kind))


@pytest.mark.parametrize("kind", [item.ITEM_F32, item.ITEM_I16])
@pytest.mark.parametrize("n,R", SHAPES)
def test_logits_backward(n, R, kind):
    check_backward(case(n, R, kind))


@pytest.mark.parametrize("R", [12, 257])
def test_share_reads_one_set_for_consecutive_rows(R):
    c = case(6, R, item.ITEM_F32, share=3)  # rows 0-2 read set 0, rows 3-5 set 1
    assert c.sets.shape[0] == 2 and not torch.equal(c.sets[0], c.sets[1])
    got = check_logits(c)
    check_backward(c)
    spread = item.item_logits(c.sets.repeat_interleave(3, 0), c.pq, c.mask, c.mask_off)  # a set of its own per row
    assert torch.equal(spread.reshape(6, c.H, R + 1), got)
    shared = item.item_logits(c.items, c.pq, c.mask, c.mask_off, share=3)
    assert torch.equal(shared.reshape(6, c.H, R + 1), got)


@pytest.mark.parametrize("n,R,kind", [(5, 12, item.ITEM_F32), (5, 1024, item.ITEM_F32), (9, 257, item.ITEM_I16)])
def test_autograd_function_returns_the_kernels_gradient_to_the_query(n, R, kind):
    c = case(n, R, kind)
    enc = item.ItemEncoder(64, fused=True).to(DEV)
    q = torch.randn((n, c.H, 64), device=DEV, requires_grad=True)
    pq = enc.pointer_query(q)
    pq.retain_grad()
    out = item.item_logits(c.items, pq, c.mask, c.mask_off)
    assert out.shape == (n, c.H * (R + 1))
    g = torch.randn_like(out)
    out.backward(g)
    g_out = torch.full((n, c.out_stride), float("nan"), dtype=torch.float32, device=DEV)
    for h, o in enumerate(c.out_off):
        g_out[:, o:o + R + 1] = g[:, h * (R + 1):(h + 1) * (R + 1)]
    keep, c.pq = c.pq, pq.detach()
    try:
        assert torch.equal(c.head_slices(c.logits()), out.detach().reshape(n, c.H, R + 1))
        assert torch.equal(c.backward(g_out).view(torch.int32), pq.grad.view(torch.int32))
    finally:
        c.pq = keep
    assert pq.grad.abs().sum() > 0
    for t in (q.grad, enc.fc.weight.grad, enc.fc.bias.grad):
        assert t is not None and bool(torch.isfinite(t).all()) and t.abs().sum() > 0


def test_the_engines_saturated_obs_rows():
    """The three comparisons on the engine's own obs buffer: a saturated state of
    tests/obs_scenarios.py installed with set_state + observe, Inventory [12, 16] with the four
    inventory heads and Market [1024, 16] with Buy, masks read from the rows' prefix."""
    from nmmo_amd import abi
    from nmmo_amd.engine import NmmoEngine
    from tests import obs_scenarios as sc

    blob = sc.state(sc.reset_blob(sc.config()), [sc.saturated()] * sc.N_ENVS)
    eng = NmmoEngine(sc.config(128, 256, obs_layout=abi.OBS_FLAT), sc.N_ENVS, seed=3)
    sc.set_tasks(eng, 128)
    eng.set_state(blob)
    eng.observe()
    lay = layout.flat_layout()
    obs = eng.obs.reshape(-1, lay["__total__"].offset)
    n = obs.shape[0]
    rng = np.random.default_rng(5)
    for name, head_names in (("Inventory", ("Destroy.InventoryItem", "Give.InventoryItem", "Sell.InventoryItem",
                                            "Use.InventoryItem")), ("Market", ("Buy.MarketItem",))):
        R = lay[name].shape[0]
        c = Case.__new__(Case)
        c.n, c.R, c.H, c.kind, c.share = n, R, len(head_names), item.ITEM_F32, 1
        c.buf, c.keep, c.mask = obs, obs.clone(), obs
        c.items = obs[:, lay[name].offset:lay[name].offset + 16 * R]
        c.sets = c.items.reshape(n, R, 16).clone()
        assert int((c.sets[:, :, 0] != 0).sum()) > 0, f"no item in any {name} section"
        c.mask_off = [lay[f"ActionTargets.{h}"].offset for h in head_names]
        c.legal = torch.stack([obs[:, o:o + R + 1] > 0 for o in c.mask_off], 1)
        c.pq = torch.from_numpy(rng.standard_normal((n, c.H, 36)).astype(np.float32)).to(DEV)
        c.out_off = [1 + h * (R + 2) for h in range(c.H)]
        c.out_stride = 1 + c.H * (R + 2) + 4
        print(f"{name}: items {int((c.sets[:, :, 0] != 0).sum())}, legal candidates {int(c.legal[..., :R].sum())}")
        if name == "Inventory":
            assert int(c.legal[..., :R].sum()) > 0
        check_features_and_sums(c.items, c.sets)
        check_logits(c)
        check_backward(c)
    assert eng.get_fault() == 0
    eng.close()
