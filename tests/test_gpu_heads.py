"""The fused masked action heads (nmmo_amd/heads.py, csrc/heads.hip) on MI355X against SPEC.md §15.

The yardstick is a float64 numpy closed form of §15 (`closed_form`, `closed_grad`) and a numpy
philox restated from csrc/common.h. Tolerances are not fixed numbers: `E_ref` is the max abs
error, over the batch, of the unfused torch float32 expressions (the loop of `masked_fill` +
`Categorical` in `MaskedLinearAgent.forward`, run on the GPU on the same inputs) against the closed
form, and the fused path must stay within 4 x E_ref — both are float32 evaluations of one formula,
the factor covers reduction order and the exp / log implementations, and a wrong offset, mask or
head gives errors of order 0.1 and up. The row with the illegal given action has a logprob near
-1e9, where one float32 ulp is 64: it gets an E_ref of its own instead of lending its error to
every other row.
"""

import ctypes

import numpy as np
import pytest
import torch

from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

NMMO_DIMS = [3, 101, 1025, 13, 13, 101, 99, 101, 5, 13, 99, 13]
LANE_DIMS = [1, 2, 63, 64, 65, 127, 128, 129, 1024, 1025, 2048]
OBS_ELEMS = 23987
BUY = 2  # the 1025-entry head
DELTA = 1e-4  # (n - 1) 2^-24 = 6.1e-5 for n = 1025 (worst-case float32 summation) + a few ulp of exp


# ---------------------------------------------------------------- the yardsticks
def philox_np(c0, c1, c2, c3, k0, k1):
    """csrc/common.h `philox` (Philox4x32-10) on uint64 arrays holding 32-bit values; returns .x"""
    c0, c1, c2, c3, k0, k1 = [np.asarray(v, dtype=np.uint64) for v in np.broadcast_arrays(c0, c1, c2, c3, k0, k1)]
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & m32, p0 & m32, n0, n2
        k0 = (k0 + np.uint64(0x9E3779B9)) & m32
        k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    return c0


def uniforms(n_rows, n_heads, seed, offset, row_base):
    r = (np.arange(n_rows, dtype=np.uint64)[:, None] + np.uint64(row_base)) & np.uint64(0xFFFFFFFF)
    k = np.arange(n_heads, dtype=np.uint64)[None, :]
    x = philox_np(r, k, offset & 0xFFFFFFFF, offset >> 32, seed & 0xFFFFFFFF, seed >> 32)
    return (x >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def head_slices(dims):
    off = np.cumsum([0] + list(dims))
    return [slice(int(off[k]), int(off[k + 1])) for k in range(len(dims))]


def closed_form(logits, legal, dims, actions):
    """SPEC §15 in float64: logprob [N], entropy [N], lse [N, H], head_entropy [N, H]."""
    x = logits.astype(np.float64)
    n, h = x.shape[0], len(dims)
    lse, hent, lp = np.zeros((n, h)), np.zeros((n, h)), np.zeros((n, h))
    for k, sl in enumerate(head_slices(dims)):
        for r in range(n):
            m = legal[r, sl]
            if not m.any():
                continue
            xs = x[r, sl][m]
            mx = xs.max()
            lse[r, k] = mx + np.log(np.exp(xs - mx).sum())
            p = np.exp(xs - lse[r, k])
            hent[r, k] = lse[r, k] - (p * xs).sum()
            a = int(actions[r, k])
            lp[r, k] = (x[r, sl][a] if m[a] else -1e9) - lse[r, k]
    return lp.sum(1), hent.sum(1), lse, hent


def closed_grad(logits, legal, dims, actions, g_logprob, g_entropy):
    """SPEC §15 backward in float64: [N, sum(dims)]."""
    x = logits.astype(np.float64)
    _, _, lse, hent = closed_form(logits, legal, dims, actions)
    g = np.zeros_like(x)
    for k, sl in enumerate(head_slices(dims)):
        m = legal[:, sl]
        logp = np.where(m, x[:, sl] - lse[:, k:k + 1], 0.0)
        p = np.where(m, np.exp(logp), 0.0)
        onehot = np.arange(sl.stop - sl.start)[None, :] == actions[:, k:k + 1]
        gk = g_logprob[:, None] * (onehot - p) - g_entropy[:, None] * p * (logp + hent[:, k:k + 1])
        g[:, sl] = np.where(m, gk, 0.0)
    return g


def torch_heads(logits, obs, dims, action):
    """The unfused expressions of MaskedLinearAgent.forward, plus per-head lse and entropy."""
    off = np.cumsum([0] + list(dims)).tolist()
    masks = obs[:, :off[-1]] > 0
    logp, ent, lses, ents = 0.0, 0.0, [], []
    for k in range(len(dims)):
        lo, hi = off[k], off[k + 1]
        lg = logits[:, lo:hi].masked_fill(~masks[:, lo:hi], -1e9)
        dist = torch.distributions.Categorical(logits=lg)
        logp = logp + dist.log_prob(action[:, k])
        e = dist.entropy()
        ent = ent + e
        lses.append(torch.logsumexp(lg, 1))
        ents.append(e)
    return logp, ent, torch.stack(lses, 1), torch.stack(ents, 1)


# ---------------------------------------------------------------- shared inputs
class Case:
    def __init__(self, name, dims, n_rows, scale, seed):
        rng = np.random.default_rng(seed)
        self.name, self.dims, self.n, self.total = name, list(dims), n_rows, int(sum(dims))
        self.slices = head_slices(dims)
        legal = rng.random((n_rows, self.total)) < 0.3
        legal[0] = False                    # all-zero: every head empty (an agent not in the realm)
        legal[1] = True                     # all-ones
        legal[2] = legal[3] = False
        for sl in self.slices:
            legal[2, sl.start] = True       # exactly the first entry of each head
            legal[3, sl.stop - 1] = True    # exactly the last entry of each head
        self.illegal = None
        if name == "nmmo":
            legal[4, self.slices[BUY]] = False  # a living row whose Buy head alone is empty
            legal[4, self.slices[0]] = True
            legal[5, self.slices[1].start + 7] = False  # row 5, head 1: the given action 7 is illegal,
            legal[5, self.slices[1].start + 8] = True   # the head is not empty
            self.illegal = (5, 1, 7)
        self.legal = legal
        self.logits_np = (rng.standard_normal((n_rows, self.total)) * scale).astype(np.float32)
        # the mask as the prefix of flat obs rows: legal iff > 0; the rest of the row is not mask
        obs = rng.standard_normal((n_rows, max(OBS_ELEMS, self.total + 5))).astype(np.float32)
        obs[:, :self.total] = np.where(legal, rng.choice([1.0, 0.5], legal.shape), rng.choice([0.0, -1.0], legal.shape))
        actions = np.zeros((n_rows, len(dims)), dtype=np.int64)
        for r in range(n_rows):
            for k, sl in enumerate(self.slices):
                idx = np.flatnonzero(legal[r, sl])
                actions[r, k] = rng.choice(idx) if len(idx) else rng.integers(sl.stop - sl.start)
        if self.illegal:
            r, k, a = self.illegal
            actions[r, k] = a
        self.actions_np = actions
        self.logits = torch.from_numpy(self.logits_np).cuda()
        self.obs = torch.from_numpy(obs).cuda()
        self.actions = torch.from_numpy(actions).cuda()
        self.g_logprob_np = rng.standard_normal(n_rows).astype(np.float32)
        self.g_entropy_np = rng.standard_normal(n_rows).astype(np.float32)
        self.ordinary = np.ones(n_rows, dtype=bool)  # rows whose logprob is not near -1e9
        if self.illegal:
            self.ordinary[self.illegal[0]] = False
        self.empty = np.array([[not legal[r, sl].any() for sl in self.slices] for r in range(n_rows)])
        # references, computed once
        self.ref = closed_form(self.logits_np, legal, dims, actions)
        with torch.no_grad():
            self.torch_fwd = [t.double().cpu().numpy() for t in torch_heads(self.logits, self.obs, dims, self.actions)]
        self._grads = {}

    def grad_refs(self, use_lp, use_ent):
        """(closed-form gradient, torch autograd gradient of the float32 expressions)"""
        key = (use_lp, use_ent)
        if key not in self._grads:
            glp = self.g_logprob_np if use_lp else np.zeros(self.n, np.float32)
            gen = self.g_entropy_np if use_ent else np.zeros(self.n, np.float32)
            want = closed_grad(self.logits_np, self.legal, self.dims, self.actions_np, glp.astype(np.float64),
                               gen.astype(np.float64))
            x = self.logits.clone().requires_grad_(True)
            logp, ent, _, _ = torch_heads(x, self.obs, self.dims, self.actions)
            loss = (logp * torch.from_numpy(glp).cuda()).sum() + (ent * torch.from_numpy(gen).cuda()).sum()
            loss.backward()
            self._grads[key] = (want, x.grad.double().cpu().numpy())
        return self._grads[key]


_cases = {}


def get_case(name):
    if name not in _cases:
        spec = {"nmmo-s1": ("nmmo", NMMO_DIMS, 37, 1.0, 11), "nmmo-s10": ("nmmo", NMMO_DIMS, 37, 10.0, 12),
                "lanes": ("lanes", LANE_DIMS, 5, 1.0, 13)}[name]
        _cases[name] = Case(*spec)
    return _cases[name]


CASES = ["nmmo-s1", "nmmo-s10", "lanes"]


def within(name, got, want, ref_got, rows=None, factor=4.0):
    """assert max|got - want| <= factor * max|ref_got - want| (over `rows`), printing both first"""
    if rows is not None:
        got, want, ref_got = got[rows], want[rows], ref_got[rows]
    err = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want)))
    e_ref = float(np.max(np.abs(ref_got - want)))
    print(f"{name}: fused err {err:.3e}  E_ref {e_ref:.3e}  bound {factor * e_ref:.3e}")
    assert np.all(np.isfinite(np.asarray(got, dtype=np.float64))), name
    assert err <= factor * e_ref, (name, err, e_ref)
    return err, e_ref


# ---------------------------------------------------------------- 1. given actions
@pytest.mark.parametrize("name", CASES)
def test_given_actions_match_closed_form(name):
    from nmmo_amd.heads import masked_heads_full

    c = get_case(name)
    a, logprob, entropy, lse, hent = masked_heads_full(c.logits, c.obs, c.dims, c.actions)
    assert a is c.actions
    got = [t.double().cpu().numpy() for t in (logprob, entropy, lse, hent)]
    want_lp, want_ent, want_lse, want_hent = c.ref
    t_lp, t_ent, t_lse, t_hent = c.torch_fwd
    o = c.ordinary
    within(f"{name} logprob", got[0], want_lp, t_lp, rows=o)
    if c.illegal:
        r = c.illegal[0]
        assert got[0][r] < -9e8
        within(f"{name} logprob (illegal action row)", got[0], want_lp, t_lp, rows=~o)
    within(f"{name} entropy", got[1], want_ent, t_ent)
    ne = ~c.empty  # torch's lse of an empty head is -1e9 + log n; §15 defines it (and the entropy) as 0
    within(f"{name} lse", got[2][ne], want_lse[ne], t_lse[ne])
    within(f"{name} head_entropy", got[3][ne], want_hent[ne], t_hent[ne])
    assert np.all(got[2][c.empty] == 0) and np.all(got[3][c.empty] == 0)
    # an empty head contributes exactly nothing: the all-zero row is 0, 0
    assert got[0][0] == 0 and got[1][0] == 0


# ---------------------------------------------------------------- 2. mask kinds
@pytest.mark.parametrize("name", CASES)
def test_mask_kinds_are_bit_identical(name):
    from nmmo_amd.heads import masked_heads_full

    c = get_case(name)
    u8 = torch.from_numpy(c.legal.astype(np.uint8)).cuda()
    for action, kw in ((c.actions, {}), (None, dict(seed=5, offset=9, row_base=2))):
        base = masked_heads_full(c.logits, c.obs, c.dims, action, **kw)
        for m in (u8, u8.bool(), torch.nn.functional.pad(u8, (0, 3), value=1)[:, :c.total + 1]):
            out = masked_heads_full(c.logits, m, c.dims, action, **kw)
            for x, y in zip(base, out):
                assert torch.equal(x, y)
    x1 = c.logits.clone().requires_grad_(True)
    x2 = c.logits.clone().requires_grad_(True)
    for x, m in ((x1, c.obs), (x2, u8.bool())):
        _, lp, ent, _, _ = masked_heads_full(x, m, c.dims, c.actions)
        (lp.sum() + 0.5 * ent.sum()).backward()
    assert torch.equal(x1.grad, x2.grad)


# ---------------------------------------------------------------- 3. sampling
def check_samples(c, actions, seed, offset, row_base):
    a = actions.cpu().numpy()
    assert a.dtype == np.int32 and a.shape == (c.n, len(c.dims))
    u = uniforms(c.n, len(c.dims), seed, offset, row_base)
    x = c.logits_np.astype(np.float64)
    worst = 0.0
    for k, sl in enumerate(c.slices):
        n = sl.stop - sl.start
        for r in range(c.n):
            m = c.legal[r, sl]
            ar = int(a[r, k])
            assert 0 <= ar < n
            if m.any():
                assert m[ar], (r, k, ar)
                e = np.where(m, np.exp(x[r, sl] - x[r, sl][m].max()), 0.0)
                cdf = np.cumsum(e) / e.sum()
            else:
                cdf = np.arange(1, n + 1) / n
            lo = cdf[ar - 1] if ar else 0.0
            worst = max(worst, lo - u[r, k], u[r, k] - cdf[ar])
            assert lo - DELTA <= u[r, k] < cdf[ar] + DELTA, (r, k, ar, lo, u[r, k], cdf[ar])
    print(f"{c.name}: worst CDF slack used {max(worst, 0.0):.3e} of {DELTA}")


@pytest.mark.parametrize("name", CASES)
def test_sampling_inverts_the_cdf(name):
    from nmmo_amd.heads import masked_heads_full

    c = get_case(name)
    seed, offset = 0x1234567887654321, (3 << 32) + 17
    a, logprob, entropy, lse, hent = masked_heads_full(c.logits, c.obs, c.dims, seed=seed, offset=offset, row_base=0)
    check_samples(c, a, seed, offset, 0)
    # the sampled call reports the sampled actions' logprob: the same as evaluating them
    _, lp2, ent2, lse2, hent2 = masked_heads_full(c.logits, c.obs, c.dims, a)
    for x, y in ((logprob, lp2), (entropy, ent2), (lse, lse2), (hent, hent2)):
        assert torch.equal(x, y)
    # same (seed, offset, row_base) -> same actions; another offset / row_base / seed -> other actions
    again = masked_heads_full(c.logits, c.obs, c.dims, seed=seed, offset=offset, row_base=0)[0]
    assert torch.equal(a, again)
    for kw in (dict(seed=seed, offset=offset + 1, row_base=0), dict(seed=seed, offset=offset, row_base=1),
               dict(seed=seed + 1, offset=offset, row_base=0), dict(seed=seed, offset=offset + (1 << 32), row_base=0)):
        other = masked_heads_full(c.logits, c.obs, c.dims, **kw)[0]
        assert not torch.equal(a, other), kw
        check_samples(c, other, kw["seed"], kw["offset"], kw["row_base"])
    # row_base = b on rows [b:] is the tail of the full call
    b = 3
    tail = masked_heads_full(c.logits[b:], c.obs[b:], c.dims, seed=seed, offset=offset, row_base=b)[0]
    assert torch.equal(tail, a[b:])


def test_sampling_picks_a_60_nat_peak():
    from nmmo_amd.heads import masked_heads

    rng = np.random.default_rng(3)
    for dims in (NMMO_DIMS, LANE_DIMS):
        n, total = 9, sum(dims)
        logits = np.full((n, total), -60.0, dtype=np.float32)
        peak = np.stack([rng.integers(d, size=n) for d in dims], 1)
        for k, sl in enumerate(head_slices(dims)):
            logits[np.arange(n), sl.start + peak[:, k]] = 0.0
        mask = torch.ones((n, total), dtype=torch.uint8, device="cuda")
        a, _, _ = masked_heads(torch.from_numpy(logits).cuda(), mask, dims, seed=7, offset=1)
        assert np.array_equal(a.cpu().numpy(), peak)


# ---------------------------------------------------------------- 4. backward
@pytest.mark.parametrize("use_lp,use_ent", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("name", CASES)
def test_backward_matches_closed_form(name, use_lp, use_ent):
    from nmmo_amd.heads import masked_heads

    c = get_case(name)
    want, torch_grad = c.grad_refs(use_lp, use_ent)
    x = c.logits.clone().requires_grad_(True)
    _, lp, ent = masked_heads(x, c.obs, c.dims, c.actions)
    loss = 0.0
    if use_lp:  # the unused output's gradient reaches backward as None
        loss = loss + (lp * torch.from_numpy(c.g_logprob_np).cuda()).sum()
    if use_ent:
        loss = loss + (ent * torch.from_numpy(c.g_entropy_np).cuda()).sum()
    loss.backward()
    got = x.grad.double().cpu().numpy()
    within(f"{name} g_logits (logprob={use_lp}, entropy={use_ent})", got, want, torch_grad)
    assert np.all(got[~c.legal] == 0)  # masked entries, and with them whole empty heads, exactly 0
    assert np.all(got[0] == 0)


@pytest.mark.parametrize("name", CASES)
def test_backward_writes_every_entry(name):
    """nmh_backward into a NaN-filled buffer with a row stride wider than sum(dims): every entry of
    the prefix is written (no pre-zeroing by the caller), the padding is not touched."""
    from nmmo_amd import heads

    c = get_case(name)
    _, _, _, lse, hent = heads.masked_heads_full(c.logits, c.obs, c.dims, c.actions)
    a32 = c.actions.to(torch.int32).contiguous()
    glp = torch.from_numpy(c.g_logprob_np).cuda()
    gen = torch.from_numpy(c.g_entropy_np).cuda()
    pad = 3
    g = torch.full((c.n, c.total + pad), float("nan"), dtype=torch.float32, device="cuda")
    hd = heads.heads_struct(c.dims)
    rc = heads.lib().nmh_backward(
        ctypes.byref(hd), c.n, c.logits.data_ptr(), c.total, c.obs.data_ptr(), c.obs.stride(0), heads.MASK_F32,
        a32.data_ptr(), lse.data_ptr(), hent.data_ptr(), glp.data_ptr(), gen.data_ptr(), g.data_ptr(), c.total + pad,
        torch.cuda.current_stream().cuda_stream)
    heads.check(rc, "nmh_backward")
    torch.cuda.synchronize()
    got = g.cpu().numpy()
    assert not np.isnan(got[:, :c.total]).any()
    assert np.isnan(got[:, c.total:]).all()
    want, torch_grad = c.grad_refs(True, True)
    within(f"{name} g_logits (raw call)", got[:, :c.total].astype(np.float64), want, torch_grad)
