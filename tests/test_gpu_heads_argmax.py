"""Greedy selection in the fused heads (SPEC.md §24; nmh_forward_argmax, nmh_pointer_forward_argmax,
nmh_decoder_forward_argmax through `masked_heads` / `pointer_heads` / `decoder_heads` with
`greedy=True`) on MI355X.

Two assertions throughout, neither with a tolerance. The actions equal numpy's first argmax over the
legal entries of the logits the head is staged from (0 where a head has none): `np.argmax` returns the
first maximum, which is §24's tie rule. And logprob, entropy, lse and head_entropy are bit for bit
(`torch.equal`) what the same entry point returns when it evaluates those actions: greedy replaces the
draw and nothing else. Gradients through a greedy call equal those through that evaluate call.

The reduction takes a per-lane first maximum (lane l owns entries [l c, (l + 1) c), c = ceil(n / 64) | 1),
a wave maximum and the lowest lane that attains it, so the shapes are the smallest that cover one
entry, fewer entries than lanes, one per lane and chunks c = 1, 3 and 17, at row counts that are not
multiples of the four rows of a workgroup. Logits come from five values so that ties are everywhere,
and row 0 carries one planted case per head (`plant`).

Pointer heads: the logits are never materialised, so the reference logits come from the existing
calls on inputs where they are the same bits: `matmul` on keys and queries from {-8..8}/8, whose dot
products are exact in any order (test_gpu_pointer_heads.py), and `item_logits` / `player_logits`, which
§23 makes bit-identical to the decoder's tile. Candidates are repeated in pairs so that equal pointer
logits occur at the maximum."""

import numpy as np
import pytest
import torch

from tests.conftest import gpu_available
from tests.test_gpu_heads import head_slices
from tests import test_gpu_decoder as dec
from tests import test_gpu_pointer_heads as ptr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

DIMS = [1, 3, 5, 64, 99, 101, 1025]
CHUNK = [((n + 63) >> 6) | 1 for n in DIMS]
VALUES = np.array([-1.0, 0.0, 0.5, 1.0, 2.0], dtype=np.float32)
ROWS = 7
K1, K3, K5, K64, K99, K101, K1025 = range(7)


def first_argmax(logits, legal, dims):
    """[N, H]: per head the smallest legal index whose logit is the largest legal logit, 0 if none."""
    x = np.where(legal, logits, -np.inf)
    return np.stack([x[:, sl].argmax(1) for sl in head_slices(dims)], 1)


def ties_at_the_maximum(logits, legal, slices, heads):
    """The number of (row, head) over `heads` whose largest legal logit is attained more than once."""
    tied = 0
    for r in range(len(logits)):
        for k in heads:
            v = np.where(legal[r, slices[k]], logits[r, slices[k]], -np.inf)
            tied += bool(legal[r, slices[k]].any()) and int((v == v.max()).sum()) > 1
    return tied


def plant(logits, legal):
    """Row 0: one case per head. Every other entry of a planted head is at most 1.0 where the plant is 2.0."""
    sl = head_slices(DIMS)
    for k in (K64, K99, K101, K1025):
        row = logits[0, sl[k]]
        row[row == 2.0] = 1.0
        legal[0, sl[k]] = True
    x, m = logits[0], legal[0]
    x[sl[K1025].start + 20] = x[sl[K1025].start + 500] = 2.0   # a maximum shared by lanes 1 and 29 (c = 17)
    x[sl[K101].start + 3] = x[sl[K101].start + 5] = 2.0        # ... shared within lane 1 (c = 3: entries 3..5)
    x[sl[K99].start + 98] = 2.0                                # ... in the last lane that has entries only
    x[sl[K64].start + 10] = 2.0                                # an illegal maximum over smaller legal values
    m[sl[K64].start + 10] = False
    m[sl[K5]] = False                                          # a head with no legal entry
    m[sl[K3]] = [False, False, True]                           # a head with only its last entry legal
    return {K1025: 20, K101: 3, K99: 98, K5: 0, K3: 2}


@pytest.fixture(scope="module")
def batch():
    rng = np.random.default_rng(24)
    total = sum(DIMS)
    logits = VALUES[rng.integers(len(VALUES), size=(ROWS, total))]
    legal = rng.random((ROWS, total)) < 0.5
    legal[1] = True
    planted = plant(logits, legal)
    want = first_argmax(logits, legal, DIMS)
    # the inputs do exercise the rules: the planted answers; an illegal maximum; and a first maximum in
    # another lane than a later equal one, in a head with c = 1, c = 3 and c = 17
    for k, a in planted.items():
        assert want[0, k] == a, (k, want[0, k])
    sl = head_slices(DIMS)
    assert logits[0, sl[K64]][want[0, K64]] < 2.0 and legal[0, sl[K64].start + want[0, K64]]
    crossed = set()
    for r in range(ROWS):
        for k, s in enumerate(sl):
            x = np.where(legal[r, s], logits[r, s], -np.inf)
            at = np.flatnonzero(x == x.max()) if legal[r, s].any() else []
            if len(at) > 1 and at[-1] // CHUNK[k] != at[0] // CHUNK[k]:
                crossed.add(CHUNK[k])
    assert crossed == {1, 3, 17}, crossed
    wide = torch.zeros((ROWS, total + 7), dtype=torch.float32, device="cuda")
    wide[:, :total] = torch.from_numpy(logits).cuda()
    f32 = torch.from_numpy(np.where(legal, rng.choice([1.0, 0.5], legal.shape), rng.choice([0.0, -1.0], legal.shape))
                           .astype(np.float32)).cuda()
    return dict(logits=wide[:, :total].contiguous(), strided=wide[:, :total], legal=legal, want=want,
                masks={"f32": f32, "u8": torch.from_numpy(legal.astype(np.uint8)).cuda()})


@pytest.mark.parametrize("view", ["contiguous", "strided"])
@pytest.mark.parametrize("kind", ["f32", "u8"])
@pytest.mark.parametrize("n", [1, 5, 7])
def test_dense_heads_select_the_first_legal_maximum(batch, n, kind, view):
    from nmmo_amd.heads import masked_heads_full

    logits = (batch["logits"] if view == "contiguous" else batch["strided"])[:n]
    assert view == "contiguous" or logits.stride(0) == sum(DIMS) + 7
    mask = batch["masks"][kind][:n]
    a, logprob, entropy, lse, hent = masked_heads_full(logits, mask, DIMS, greedy=True, seed=9, offset=3)
    assert a.dtype == torch.int32 and tuple(a.shape) == (n, len(DIMS))
    got = a.cpu().numpy()
    print(f"n={n} {kind} {view}: {int((got != batch['want'][:n]).sum())} of {got.size} actions differ")
    assert np.array_equal(got, batch["want"][:n])
    given = masked_heads_full(logits, mask, DIMS, a)
    for name, x, y in zip(("logprob", "entropy", "lse", "head_entropy"), (logprob, entropy, lse, hent), given[1:]):
        assert torch.equal(x, y), name
    # where every legal logit is above -1e9 this is the reference's argmax(masked_fill(mask == 0, -1e9))
    legal = torch.from_numpy(batch["legal"][:n]).cuda()
    for k, sl in enumerate(head_slices(DIMS)):
        assert torch.equal(logits[:, sl].masked_fill(~legal[:, sl], -1e9).argmax(1).to(torch.int32), a[:, k]), k
    sl = head_slices(DIMS)[K5]  # the empty head contributes nothing
    assert float(lse[0, K5]) == 0.0 and float(hent[0, K5]) == 0.0 and not batch["legal"][0, sl].any()


def test_dense_greedy_backward_is_the_evaluate_calls(batch):
    from nmmo_amd.heads import masked_heads

    g = torch.Generator().manual_seed(1)
    glp, gen = torch.randn(ROWS, generator=g).cuda(), torch.randn(ROWS, generator=g).cuda()
    grads = []
    action = None
    for _ in range(2):
        x = batch["logits"].clone().requires_grad_(True)
        a, lp, ent = masked_heads(x, batch["masks"]["u8"], DIMS, action, greedy=action is None)
        ((lp * glp).sum() + (ent * gen).sum()).backward()
        grads.append(x.grad)
        action = a
    assert torch.equal(grads[0], grads[1]) and float(grads[0].abs().max()) > 0


# ---------------------------------------------------------------- pointer heads
class PointerInputs:
    """A test_gpu_pointer_heads case's shapes and masks with keys, queries and dense logits of this
    file: values from {-8..8}/8 (every dot product exact), candidate 2 i + 1 a copy of candidate 2 i."""

    def __init__(self, name):
        c = ptr.get_case(name)  # shared and left unchanged
        rng = np.random.default_rng(sum(map(ord, name)) + 24)
        grid = lambda *shape: torch.from_numpy((rng.integers(-8, 9, shape) / 8.0).astype(np.float32))  # noqa: E731
        self.c = c
        self.queries = grid(c.n, len(c.ptr), c.D).cuda()
        self.keys = []
        for m in c.set_rows:
            k = grid(c.n, m, c.D)
            k[:, 1::2] = k[:, 0:m - m % 2:2]
            self.keys.append(k.cuda())
        n_dense = len(c.dense_cols)
        self.dense = grid(c.n, n_dense).cuda() if n_dense else None
        with torch.no_grad():
            self.logits = ptr.materialise(self.queries, self.keys, c.head_set, self.dense, c.dims)
        self.want = first_argmax(self.logits.cpu().numpy(), c.legal, c.dims)

    def call(self, kind, action=None, greedy=False, leaves=None):
        from nmmo_amd.heads import pointer_heads_full

        q, keys, d = leaves if leaves else (self.queries, self.keys, self.dense)
        return pointer_heads_full(q, keys, self.c.head_set, d, self.c.mask(kind), self.c.dims, action, greedy=greedy)


_pointer = {}


def pointer_inputs(name):
    if name not in _pointer:
        _pointer[name] = PointerInputs(name)
    return _pointer[name]


POINTER = ["all-pointer", "wide"]  # 7 rows, D = 72 (two chunks of a key row); 5 rows with dense heads, D = 256


@pytest.mark.parametrize("name", POINTER)
def test_pointer_inputs_tie_at_the_maximum(name):
    p = pointer_inputs(name)
    tied = ties_at_the_maximum(p.logits.cpu().numpy(), p.c.legal, p.c.slices, p.c.ptr)
    assert tied >= 2, tied


@pytest.mark.parametrize("kind", ["f32", "u8"])
@pytest.mark.parametrize("name", POINTER)
def test_pointer_heads_select_the_first_legal_maximum(name, kind):
    p = pointer_inputs(name)
    with torch.no_grad():
        a, logprob, entropy, lse, hent = p.call(kind, greedy=True)
        given = p.call(kind, action=a)
    got = a.cpu().numpy()
    print(f"{name} {kind}: {int((got != p.want).sum())} of {got.size} actions differ")
    assert a.dtype == torch.int32 and np.array_equal(got, p.want)
    for what, x, y in zip(("logprob", "entropy", "lse", "head_entropy"), (logprob, entropy, lse, hent), given[1:]):
        assert torch.equal(x, y), what
    assert np.all(got[p.c.empty] == 0)


@pytest.mark.parametrize("name", POINTER)
def test_pointer_greedy_backward_is_the_evaluate_calls(name):
    p = pointer_inputs(name)
    g = torch.Generator().manual_seed(2)
    glp, gen = torch.randn(p.c.n, generator=g).cuda(), torch.randn(p.c.n, generator=g).cuda()
    grads, action = [], None
    for _ in range(2):
        leaves = (p.queries.clone().requires_grad_(True), [k.clone().requires_grad_(True) for k in p.keys],
                  None if p.dense is None else p.dense.clone().requires_grad_(True))
        out = p.call("f32", action=action, greedy=action is None, leaves=leaves)
        ((out[1] * glp).sum() + (out[2] * gen).sum()).backward()
        grads.append([leaves[0].grad, *[k.grad for k in leaves[1]], *([] if leaves[2] is None else [leaves[2].grad])])
        action = out[0]
    assert all(torch.equal(x, y) for x, y in zip(*grads)) and len(grads[0]) == len(grads[1])
    assert float(grads[0][0].abs().max()) > 0


# ---------------------------------------------------------------- decoder
class DecoderInputs:
    """test_gpu_decoder.py's synthetic A at 5 rows (entity sets of 65 and 256, item sets of 1 and 64; its
    own instance, so the shared ones stay as they are) with candidate 2 i + 1 of every set a copy of
    candidate 2 i, in the float32 rows and in their int16 copy."""

    def __init__(self):
        c = dec.Case("A", 5, seed=24)
        for buf in (c.buf, c.ibuf):
            for s, R in enumerate(c.rows):
                x = c.view(s, buf).view(c.n, R, dec.COLS[c.rules[s]])  # a view of the rows: written in place
                x[:, 1::2] = x[:, 0:R - R % 2:2].clone()
        self.c = c

    def args(self, elem):
        c = self.c
        return (c.buf, c.buf) if elem == "f32" else (c.ibuf, c.mask_u8)

    def logits(self, elem):
        """The logits row of the composed path: the dense heads as given, `item_logits` / `player_logits`."""
        from nmmo_amd.item import item_logits
        from nmmo_amd.player import player_logits

        c = self.c
        buf, mask = self.args(elem)
        parts, d = [None] * len(c.dims), 0
        for k, s in enumerate(c.head_set):
            if s < 0:
                parts[k] = c.dense[:, d:d + c.dims[k]]
                d += c.dims[k]
        for s, (rule, R) in enumerate(zip(c.rules, c.rows)):
            ks = [k for k in c.pointer if c.head_set[k] == s]
            slots = c.pq[:, [c.pointer.index(k) for k in ks], :40 if rule == dec.E else 36]
            fn = player_logits if rule == dec.E else item_logits
            lg = fn(c.view(s, buf), slots, mask, [c.slices[k].start for k in ks], set_rows=R)
            for i, k in enumerate(ks):
                parts[k] = lg[:, i * (R + 1):(i + 1) * (R + 1)]
        return torch.cat(parts, 1)

    def call(self, elem, dense=None, pq=None, action=None, greedy=False):
        from nmmo_amd.decoder import decoder_heads_full

        c = self.c
        buf, mask = self.args(elem)
        sets = [(c.view(s, buf), "entity" if rule == dec.E else "item") for s, rule in enumerate(c.rules)]
        return decoder_heads_full(c.dense if dense is None else dense, c.pq if pq is None else pq, sets, c.head_set,
                                  mask, c.dims, action, greedy=greedy)


@pytest.fixture(scope="module")
def decoder_inputs():
    return DecoderInputs()


@pytest.mark.parametrize("elem", ["f32", "i16"])
def test_decoder_heads_select_the_first_legal_maximum(decoder_inputs, elem):
    d, c = decoder_inputs, decoder_inputs.c
    with torch.no_grad():
        x = d.logits(elem).cpu().numpy()
        want = first_argmax(x, c.legal, c.dims)
        tied = ties_at_the_maximum(x, c.legal, c.slices, c.pointer)
        assert tied >= 2, tied  # equal pointer logits at the maximum do occur
        a, logprob, entropy, lse, hent = d.call(elem, greedy=True)
        given = d.call(elem, action=a)
    got = a.cpu().numpy()
    print(f"decoder {elem}: {int((got != want).sum())} of {got.size} actions differ; {tied} heads tie at the maximum")
    assert a.dtype == torch.int32 and np.array_equal(got, want)
    for what, p, q in zip(("logprob", "entropy", "lse", "head_entropy"), (logprob, entropy, lse, hent), given[1:]):
        assert torch.equal(p, q), what
    assert not c.legal[1].any() and np.all(got[1] == 0) and float(logprob[1]) == 0.0  # row 1: every head empty


def test_decoder_greedy_backward_is_the_evaluate_calls(decoder_inputs):
    d, c = decoder_inputs, decoder_inputs.c
    grads, action = [], None
    for _ in range(2):
        dense, pq = c.dense.clone().requires_grad_(True), c.pq.clone().requires_grad_(True)
        out = d.call("f32", dense, pq, action=action, greedy=action is None)
        ((out[1] * c.g_logprob).sum() + (out[2] * c.g_entropy).sum()).backward()
        grads.append((dense.grad, pq.grad))
        action = out[0]
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    assert float(grads[0][1].abs().max()) > 0
