"""The fused pointer heads (nmmo_amd/heads.py `pointer_heads`, csrc/heads.hip) on MI355X against
SPEC.md §18.

Two yardsticks. With keys and queries drawn from {-8..8}/8 every dot product is exact in float32
in any order, so the fused call must equal `masked_heads_full` on the logits materialised the
reference's way (`cat` of a zero row, `matmul`) bit for bit. With general inputs the yardstick is
test_gpu_heads.py's: a float64 restatement (numpy einsum logits, `closed_form` / `closed_grad`,
the chain rule of §18) and `within`: the fused error may be at most 4 x the error of the unfused
float32 torch chain against the same float64 values. A row with an illegal given action (logprob
near -1e9, one ulp = 64) has a bound of its own, as in test_gpu_heads.py.

General inputs: keys are standard normal and queries standard normal / sqrt(D), so logits are
standard normal. Shapes are the smallest that take every path: D = 4 / 64 (one 64-float chunk per
key row), 72 (two, the second partial), 256 (four); m = 1, 5 (a partial four-candidate pass), 12,
13, 100, 1024; 1, 4, 5, 7 and 37 rows (partial and several workgroups).

The "tiny" cases have 4 to 20 gradient entries per call, too few for a maximum over the batch to
say anything about the torch chain's error. They hold 32 or 35 rows of independent inputs and
every test feeds them to the fused path in calls of 1, 4 or 5 rows (`row_base` carries the row
index, so the draws are those of one call); errors and E_ref are maxima over all of them.
"""

import ctypes

import numpy as np
import pytest
import torch

from tests.conftest import gpu_available
from tests.test_gpu_heads import check_samples, closed_form, closed_grad, head_slices, torch_heads, within

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

NMMO_DIMS = [3, 101, 1025, 13, 13, 101, 99, 101, 5, 13, 99, 13]
NMMO_SETS = [-1, 0, 2, 1, 1, 0, -1, 0, -1, 1, -1, 1]
# name: (rows, rows per call (0: all), dims, head_set, set_rows, D)
SPECS = {
    "nmmo": (37, 0, NMMO_DIMS, NMMO_SETS, [100, 12, 1024], 64),
    "tiny-1": (32, 1, [2, 1], [0, -1], [1], 4),
    "tiny-4": (32, 4, [2, 1], [0, -1], [1], 4),
    "tiny-5": (35, 5, [2, 1], [0, -1], [1], 4),
    "wide": (5, 0, [6, 6, 3, 6, 6, 7], [0, 0, -1, 0, 0, -1], [5], 256),
    "all-pointer": (7, 0, [6, 14, 6], [0, 1, 0], [5, 13], 72),
    "no-pointer": (7, 0, [3, 5, 99], [-1, -1, -1], [], 0),
}
CASES = list(SPECS)
POINTER_CASES = [c for c in CASES if c != "no-pointer"]
# per head: empty, only the no-op, exactly one candidate, all legal, random ~50 %, random ~1 %
N_PATTERNS = 6


def head_mask(rng, n, pattern):
    legal = np.zeros(n, dtype=bool)
    if pattern == 1:
        legal[n - 1] = True
    elif pattern == 2:
        legal[rng.integers(max(n - 1, 1))] = True
    elif pattern == 3:
        legal[:] = True
    elif pattern >= 4:
        legal = rng.random(n) < (0.5 if pattern == 4 else 0.01)
    return legal


def materialise(queries, keys, head_set, dense, dims):
    """The reference's decoder: per pointer head cat(keys, zero row) @ query; dense heads as given."""
    padded = [torch.cat([k, k.new_zeros(k.shape[0], 1, k.shape[2])], 1) for k in keys]
    parts, p, d = [], 0, 0
    for n, s in zip(dims, head_set):
        if s < 0:
            parts.append(dense[:, d:d + n])
            d += n
        else:
            parts.append(torch.matmul(padded[s], queries[:, p].unsqueeze(-1)).squeeze(-1))
            p += 1
    return torch.cat(parts, 1)


class Inputs:
    """keys / queries / dense logits of one kind, their materialised float32 logits, and what
    check_samples reads of a test_gpu_heads Case."""

    def __init__(self, case, queries, keys, dense):
        self.name, self.n, self.dims, self.slices, self.legal = case.name, case.n, case.dims, case.slices, case.legal
        dev = lambda a: None if a is None else torch.from_numpy(a).cuda()  # noqa: E731
        self.queries_np, self.keys_np, self.dense_np = queries, keys, dense
        self.queries, self.keys, self.dense = dev(queries), [dev(k) for k in keys], dev(dense)
        with torch.no_grad():
            self.logits = materialise(self.queries, self.keys, case.head_set, self.dense, case.dims)
        self.logits_np = self.logits.cpu().numpy()


class Case:
    def __init__(self, name):
        n, chunk, dims, head_set, set_rows, D = SPECS[name]
        self.calls = [slice(i, min(n, i + (chunk or n))) for i in range(0, n, chunk or n)]
        rng = np.random.default_rng(sum(map(ord, name)))
        self.name, self.n, self.dims, self.head_set, self.set_rows, self.D = name, n, list(dims), head_set, set_rows, D
        self.total, self.slices = sum(dims), head_slices(dims)
        H = len(dims)
        self.ptr = [k for k in range(H) if head_set[k] >= 0]
        self.dense_cols = np.concatenate([np.arange(sl.start, sl.stop) for sl, s in zip(self.slices, head_set)
                                          if s < 0] or [np.zeros(0, dtype=np.int64)])
        # rows 0..5 hold one pattern in every head (row 0 of "nmmo": an agent not in the realm), the
        # rows after them mix the non-empty patterns over the heads; one of those gets one empty head
        legal = np.zeros((n, self.total), dtype=bool)
        for r in range(n):
            for k, sl in enumerate(self.slices):
                pattern = r if r < N_PATTERNS else 1 + (r + k) % (N_PATTERNS - 1)
                legal[r, sl] = head_mask(rng, dims[k], pattern)
        if n > N_PATTERNS:
            legal[N_PATTERNS, self.slices[min(1, H - 1)]] = False
        self.legal = legal
        self.empty = np.array([[not legal[r, sl].any() for sl in self.slices] for r in range(n)])
        # the two mask kinds: the prefix of a wider float32 obs-like row, and bytes
        obs = rng.standard_normal((n, self.total + 37)).astype(np.float32)
        obs[:, :self.total] = np.where(legal, rng.choice([1.0, 0.5], legal.shape), rng.choice([0.0, -1.0], legal.shape))
        self.obs = torch.from_numpy(obs).cuda()
        self.u8 = torch.from_numpy(legal.astype(np.uint8)).cuda()
        # a candidate row of a set is read iff it is legal in some head that points into the set
        self.row_used = []
        for s, m in enumerate(set_rows):
            used = np.zeros((n, m), dtype=bool)
            for k in self.ptr:
                if head_set[k] == s:
                    used |= legal[:, self.slices[k]][:, :m]
            self.row_used.append(used)
        # given actions: a legal one where the head has any, plus an illegal one, one past the end and a
        # negative one in three rows of their own; the references evaluate an in-range illegal entry
        # in their place (§15 gives all three the logit -1e9, and torch cannot index out of range)
        actions = np.zeros((n, H), dtype=np.int64)
        for r in range(n):
            for k, sl in enumerate(self.slices):
                idx = np.flatnonzero(legal[r, sl])
                actions[r, k] = rng.choice(idx) if len(idx) else rng.integers(dims[k])
        self.ref_actions = actions.copy()
        self.ordinary = np.ones(n, dtype=bool)
        odd = [lambda bad, k: bad, lambda bad, k: dims[k] + 3, lambda bad, k: -1]
        for r in range(n - 1, -1, -1):
            for k, sl in enumerate(self.slices):
                if odd and legal[r, sl].any() and not legal[r, sl].all():
                    bad = int(np.flatnonzero(~legal[r, sl])[0])
                    actions[r, k], self.ref_actions[r, k] = odd.pop(0)(bad, k), bad
                    self.ordinary[r] = False
                    break
        self.actions = torch.from_numpy(actions).cuda()
        self.actions_np = actions
        self.g_logprob_np = rng.standard_normal(n).astype(np.float32)
        self.g_entropy_np = rng.standard_normal(n).astype(np.float32)
        P = len(self.ptr)
        n_dense = len(self.dense_cols)
        grid = lambda *shape: (rng.integers(-8, 9, shape) / 8.0).astype(np.float32)  # noqa: E731
        normal = lambda *shape: rng.standard_normal(shape).astype(np.float32)  # noqa: E731
        self.exact = Inputs(self, grid(n, P, D) if P else None, [grid(n, m, D) for m in set_rows],
                            grid(n, n_dense) if n_dense else None)
        # general inputs; rows that no head may read are zero here and NaN in `nan_keys`
        keys = [normal(n, m, D) * used[:, :, None] for m, used in zip(set_rows, self.row_used)]
        self.general = Inputs(self, normal(n, P, D) / np.float32(np.sqrt(D)) if P else None, keys,
                              normal(n, n_dense) if n_dense else None)
        self.nan_keys = [torch.where(torch.from_numpy(used).cuda()[:, :, None], k, torch.full_like(k, float("nan")))
                         for k, used in zip(self.general.keys, self.row_used)]
        self._refs = None

    def mask(self, kind):
        return self.obs if kind == "f32" else self.u8

    def refs(self):
        """On the general inputs, once: the float64 restatement and the float32 torch chain, each as
        (logprob, entropy, lse, head_entropy, g_dense, g_queries, [g_keys])."""
        if self._refs is not None:
            return self._refs
        g, hs = self.general, self.head_set
        q64 = None if g.queries_np is None else g.queries_np.astype(np.float64)
        k64 = [k.astype(np.float64) for k in g.keys_np]
        x = np.zeros((self.n, self.total))
        if len(self.dense_cols):
            x[:, self.dense_cols] = g.dense_np
        for p, k in enumerate(self.ptr):
            sl, m = self.slices[k], self.dims[k] - 1
            x[:, sl.start:sl.start + m] = np.einsum("rjd,rd->rj", k64[hs[k]], q64[:, p])
        glp, gen = self.g_logprob_np.astype(np.float64), self.g_entropy_np.astype(np.float64)
        gx = closed_grad(x, self.legal, self.dims, self.ref_actions, glp, gen)
        gq = np.zeros_like(q64) if q64 is not None else None
        gk = [np.zeros_like(k) for k in k64]
        for p, k in enumerate(self.ptr):
            sl, m = self.slices[k], self.dims[k] - 1
            gj = gx[:, sl.start:sl.start + m]
            gq[:, p] = np.einsum("rj,rjd->rd", gj, k64[hs[k]])
            gk[hs[k]] += np.einsum("rj,rd->rjd", gj, q64[:, p])
        want = (*closed_form(x, self.legal, self.dims, self.ref_actions), gx[:, self.dense_cols], gq, gk)
        leaves = [None if t is None else t.clone().requires_grad_(True) for t in (g.queries, g.dense)]
        keys = [k.clone().requires_grad_(True) for k in g.keys]
        ref_a = torch.from_numpy(self.ref_actions).cuda()
        out = torch_heads(materialise(leaves[0], keys, hs, leaves[1], self.dims), self.obs, self.dims, ref_a)
        (out[0] * torch.from_numpy(self.g_logprob_np).cuda() + out[1] * torch.from_numpy(self.g_entropy_np).cuda()).sum().backward()
        f64 = lambda t: None if t is None else t.detach().double().cpu().numpy()  # noqa: E731
        chain = (*[f64(t) for t in out], f64(None if leaves[1] is None else leaves[1].grad),
                 f64(None if leaves[0] is None else leaves[0].grad), [f64(k.grad) for k in keys])
        self._refs = (want, chain)
        return self._refs


_cases = {}


def get_case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


def fused_calls(c, queries, keys, dense, mask, action, seed=0, offset=0, row_base=0):
    """`pointer_heads_full` on the case's rows, one call per entry of c.calls, the outputs concatenated."""
    from nmmo_amd.heads import pointer_heads_full

    cut = lambda t, sl: None if t is None else t[sl]  # noqa: E731
    outs = [pointer_heads_full(cut(queries, sl), [k[sl] for k in keys], c.head_set, cut(dense, sl), mask[sl], c.dims,
                               cut(action, sl), seed=seed, offset=offset, row_base=row_base + sl.start)
            for sl in c.calls]
    return outs[0] if len(outs) == 1 else tuple(torch.cat(t) for t in zip(*outs))


def fused(c, inp, kind="f32", action=None, keys=None, **kw):
    return fused_calls(c, inp.queries, inp.keys if keys is None else keys, inp.dense, c.mask(kind), action, **kw)


def fused_grads(c, kind="f32", keys=None):
    """(forward outputs, g_dense, g_queries, [g_keys]) of the fused path on the general inputs."""
    g = c.general
    q, d = [None if t is None else t.clone().requires_grad_(True) for t in (g.queries, g.dense)]
    ks = [k.clone().requires_grad_(True) for k in (g.keys if keys is None else keys)]
    out = fused_calls(c, q, ks, d, c.mask(kind), c.actions)
    (out[1] * torch.from_numpy(c.g_logprob_np).cuda() + out[2] * torch.from_numpy(c.g_entropy_np).cuda()).sum().backward()
    return out, None if d is None else d.grad, None if q is None else q.grad, [k.grad for k in ks]


# ---------------------------------------------------------------- 1. exact inputs
@pytest.mark.parametrize("kind", ["f32", "u8"])
@pytest.mark.parametrize("name", CASES)
def test_exact_inputs_equal_masked_heads_on_materialised_logits(name, kind):
    from nmmo_amd.heads import masked_heads_full

    c = get_case(name)
    e = c.exact
    if name == "no-pointer":
        assert torch.equal(e.logits, e.dense)
    seed, offset, row_base = 0x1234567887654321, (3 << 32) + 17, 5
    for action, kw in ((c.actions, {}), (None, dict(seed=seed, offset=offset, row_base=row_base))):
        got = fused(c, e, kind, action, **kw)
        want = masked_heads_full(e.logits, c.mask(kind), c.dims, action, **kw)
        for i, (x, y) in enumerate(zip(got, want)):
            assert torch.equal(x, y), (name, kind, "given" if action is not None else "sampled", i)
    check_samples(e, got[0], seed, offset, row_base)


# ---------------------------------------------------------------- 2. / 3. general inputs
def check_general(c, tag, out, g_dense, g_queries, g_keys):
    want, chain = c.refs()
    got = [t.detach().double().cpu().numpy() for t in out[1:]]
    o, ne = c.ordinary, ~c.empty
    within(f"{tag} logprob", got[0], want[0], chain[0], rows=o)
    within(f"{tag} entropy", got[1], want[1], chain[1])
    if (~o).any():
        assert np.all(got[0][~o] < -9e8)
        within(f"{tag} logprob (illegal action rows)", got[0], want[0], chain[0], rows=~o)
    if ne.any():
        within(f"{tag} lse", got[2][ne], want[2][ne], chain[2][ne])
        within(f"{tag} head_entropy", got[3][ne], want[3][ne], chain[3][ne])
    assert np.all(got[2][c.empty] == 0) and np.all(got[3][c.empty] == 0)
    if g_dense is not None:
        gd = g_dense.double().cpu().numpy()
        within(f"{tag} g_dense", gd, want[4], chain[4])
        assert np.all(gd[~c.legal[:, c.dense_cols]] == 0)
    if g_queries is not None:
        gq = g_queries.double().cpu().numpy()
        within(f"{tag} g_queries", gq, want[5], chain[5])
        for p, k in enumerate(c.ptr):  # no legal candidate (empty, or only the no-op): exactly 0
            none = ~c.legal[:, c.slices[k]][:, :c.dims[k] - 1].any(1)
            assert np.all(gq[none, p] == 0), k
    for s, gk in enumerate(g_keys):
        gk = gk.double().cpu().numpy()
        within(f"{tag} g_keys[{s}]", gk, want[6][s], chain[6][s])
        assert np.all(gk[~c.row_used[s]] == 0), s


@pytest.mark.parametrize("name", CASES)
def test_general_inputs_match_float64(name):
    c = get_case(name)
    out, gd, gq, gk = fused_grads(c)
    assert torch.equal(out[0], c.actions)
    check_general(c, name, out, gd, gq, gk)
    # the byte mask gives the same bits
    out8, gd8, gq8, gk8 = fused_grads(c, "u8")
    for x, y in zip([*out[1:], gd, gq, *gk], [*out8[1:], gd8, gq8, *gk8]):
        assert (x is None and y is None) or torch.equal(x, y)


@pytest.mark.parametrize("name", POINTER_CASES)
def test_illegal_key_rows_are_never_read(name):
    c = get_case(name)
    for k, used in zip(c.nan_keys, c.row_used):
        assert torch.isnan(k[torch.from_numpy(~used).cuda()]).all()
    out, gd, gq, gk = fused_grads(c, keys=c.nan_keys)
    check_general(c, name + " (NaN keys)", out, gd, gq, gk)
    # and sampling does not see them either
    a, lp, ent, _, _ = fused(c, c.general, keys=c.nan_keys, seed=3, offset=1)
    b = fused(c, c.general, seed=3, offset=1)
    assert torch.equal(a, b[0]) and torch.equal(lp, b[1]) and torch.equal(ent, b[2])
    assert torch.isfinite(lp).all() and torch.isfinite(ent).all()


# ---------------------------------------------------------------- 4. sampling on general inputs
@pytest.mark.parametrize("name", CASES)
def test_sampling_on_general_inputs(name):
    c = get_case(name)
    g = c.general
    seed, offset = 77, (1 << 32) + 5
    a, lp, ent, lse, hent = fused(c, g, seed=seed, offset=offset)
    an = a.cpu().numpy()
    assert an.dtype == np.int32 and an.shape == (c.n, len(c.dims))
    for k, sl in enumerate(c.slices):
        assert np.all((an[:, k] >= 0) & (an[:, k] < c.dims[k]))
        has = ~c.empty[:, k]
        assert np.all(c.legal[:, sl][np.arange(c.n), an[:, k]][has]), k
    again = fused(c, g, action=a)
    for x, y in zip((lp, ent, lse, hent), again[1:]):
        assert torch.equal(x, y)
    assert torch.equal(a, fused(c, g, seed=seed, offset=offset)[0])
    if c.n > 1:
        from nmmo_amd.heads import pointer_heads_full

        b = c.n // 2
        tail = pointer_heads_full(None if g.queries is None else g.queries[b:], [k[b:] for k in g.keys], c.head_set,
                                  None if g.dense is None else g.dense[b:], c.obs[b:], c.dims, seed=seed,
                                  offset=offset, row_base=b)
        assert torch.equal(tail[0], a[b:]) and torch.equal(tail[1], lp[b:])


# ---------------------------------------------------------------- 5. backward writes every entry
@pytest.mark.parametrize("name", CASES)
def test_backward_writes_every_entry_and_repeats(name):
    from nmmo_amd import heads

    c = get_case(name)
    g = c.general
    out, gd, gq, gk = fused_grads(c)
    _, _, _, lse, hent = out
    a32 = c.actions.to(torch.int32).contiguous()
    glp, gen = torch.from_numpy(c.g_logprob_np).cuda(), torch.from_numpy(c.g_entropy_np).cuda()
    nan_like = lambda t: None if t is None else torch.full_like(t, float("nan"))  # noqa: E731
    pad = 3  # g_dense with a row stride wider than the dense heads: the padding is not touched
    n_dense = len(c.dense_cols)
    raw_d = torch.full((c.n, n_dense + pad), float("nan"), device="cuda") if n_dense else None
    raw_q, raw_k = nan_like(g.queries), [nan_like(k) for k in g.keys]
    hd = heads.heads_struct(c.dims)
    pt = heads.pointer_struct(c.dims, c.head_set, c.set_rows, c.D)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    arr = lambda ts: (ctypes.c_void_p * max(1, len(ts)))(*[ptr(t) for t in ts])  # noqa: E731

    def backward(g_dense, g_queries, g_keys):
        rc = heads.lib().nmh_pointer_backward(
            ctypes.byref(hd), ctypes.byref(pt), c.n, ptr(g.queries), arr(g.keys), ptr(g.dense), n_dense,
            c.obs.data_ptr(), c.obs.stride(0), heads.MASK_F32, a32.data_ptr(), lse.data_ptr(), hent.data_ptr(),
            glp.data_ptr(), gen.data_ptr(), ptr(g_dense), n_dense + pad, ptr(g_queries), arr(g_keys),
            torch.cuda.current_stream().cuda_stream)
        heads.check(rc, "nmh_pointer_backward")
        torch.cuda.synchronize()

    backward(raw_d, raw_q, raw_k)
    if n_dense:
        assert torch.equal(raw_d[:, :n_dense], gd) and torch.isnan(raw_d[:, n_dense:]).all()
    if raw_q is not None:
        assert torch.equal(raw_q, gq)
    for s in range(len(raw_k)):
        assert not torch.isnan(raw_k[s]).any() and torch.equal(raw_k[s], gk[s]), s
    # a NULL output is left alone (here: only the last key set's gradient is asked for)
    if raw_k:
        only = [None] * (len(raw_k) - 1) + [nan_like(g.keys[-1])]
        backward(None, None, only)
        assert torch.equal(only[-1], gk[-1])
    # through autograd: keys that do not require a gradient get none, and a second run repeats the bits
    q = None if g.queries is None else g.queries.clone().requires_grad_(True)
    d = None if g.dense is None else g.dense.clone().requires_grad_(True)
    _, lp, ent, _, _ = heads.pointer_heads_full(q, g.keys, c.head_set, d, c.obs, c.dims, c.actions)
    (lp * glp + ent * gen).sum().backward()
    assert all(k.grad is None for k in g.keys)
    if q is not None:
        assert torch.equal(q.grad, gq)
    if d is not None:
        assert torch.equal(d.grad, gd)


def test_wrong_shapes_and_dtypes_raise_value_error():
    from nmmo_amd.heads import pointer_heads

    c = get_case("all-pointer")
    g = c.general
    with pytest.raises(ValueError, match="queries"):
        pointer_heads(g.queries[:, :2], g.keys, c.head_set, None, c.obs, c.dims)
    with pytest.raises(ValueError, match="queries"):
        pointer_heads(g.queries.double(), g.keys, c.head_set, None, c.obs, c.dims)
    with pytest.raises(ValueError, match="keys"):
        pointer_heads(g.queries, [g.keys[0], g.keys[1][:3]], c.head_set, None, c.obs, c.dims)
    with pytest.raises(ValueError, match="no-op"):
        pointer_heads(g.queries, [g.keys[0], g.keys[1][:, :5]], c.head_set, None, c.obs, c.dims)
    with pytest.raises(ValueError, match="dense_logits"):
        w = get_case("wide")
        pointer_heads(w.general.queries, w.general.keys, w.head_set, None, w.obs, w.dims)
    # a non-contiguous and a misaligned input are copied, not refused
    wide = torch.zeros((c.n, 3, c.D + 4), device="cuda")
    wide[:, :, 1:c.D + 1] = g.queries
    off = torch.zeros(g.keys[0].numel() + 1, device="cuda")
    off[1:] = g.keys[0].reshape(-1)
    base = fused(c, g, action=c.actions)
    out = fused(c, Shifted(g, wide[:, :, 1:c.D + 1], [off[1:].view_as(g.keys[0]), g.keys[1]]), action=c.actions)
    assert off[1:].data_ptr() % 16 == 4
    for x, y in zip(base[1:], out[1:]):
        assert torch.equal(x, y)


class Shifted:
    def __init__(self, inp, queries, keys):
        self.queries, self.keys, self.dense = queries, keys, inp.dense
