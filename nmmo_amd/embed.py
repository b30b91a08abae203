"""Entity and item sets whose discrete columns are embedding lookups: the takeru policy's
ReducedPlayerEncoder and ReducedItemEncoder (agent_zoo/takeru/policy.py:115-258) without their
[N, R, H] embeddings (nmh_embed_features / nmh_embed_logits / nmh_embed_logits_backward of
libnmmo_heads.so, include/nmmo_heads.h, SPEC.md §25).

A candidate's feature is feat = cat(E[idx_0], .., E[idx_{D-1}], x_0 / s_0, .., x_{C-1} / s_{C-1}) with
idx_d = clip(trunc(x + off_d), 0, 255), and the layer over it (`agent_fc`, `fc`) is linear, so

    q . fc(feat_j) = sum_d pq[d][idx_d(j)] + sum_c pq[cont c] x_c / s_c + pq[bias]     `embed_logits`
    mean_j fc(feat_j) = fc(cat(counts_d @ E[0:256] / R, sums / s / R))                 `embed_counts`

where `pointer_query` folds a head's query, the layer and the table into the per-row score table pq.
The kernels hold no parameters; torch autograd takes pq's gradient back to the layer and to E.

    enc = ReducedItemEncoder(64, 64, fused=True).cuda()
    market = obs[:, o_market:o_market + 1024 * 16]                 # a view, read in place
    pooled = enc.pooled(market)                                    # [N, 64]
    logits = embed_logits(ITEM, market, enc.pointer_query(q), obs, [mask_off_buy])   # [N, 1025]

There is no torch fallback for the fused path: a host tensor, or a missing library, is a `HeadsError`.
"""

from __future__ import annotations

from typing import NamedTuple

import torch
from torch import nn
from torch.nn import functional as F

from . import _sets, abi, heads
from .heads import HeadsError

BINS, EMBED = 256, 32  # table rows an index can reach (the clip comes after the offset), floats per table row
_ptr = heads.ptr


class Kind(NamedTuple):
    """An embedded set kind (SPEC.md §25), as the library's compile-time descriptors state it."""
    name: str
    code: int  # NMH_EMBED_*
    cols: int
    dcols: tuple  # the discrete columns ...
    doffs: tuple  # ... and their offsets
    ccols: tuple  # the continuous columns ...
    cdivs: tuple  # ... and their divisors
    max_rows: int
    spec: _sets.SetSpec

    D = property(lambda self: len(self.dcols))
    C = property(lambda self: len(self.ccols))
    features = property(lambda self: len(self.dcols) * EMBED + len(self.ccols))  # the linear layer's input
    bias = property(lambda self: len(self.dcols) * BINS + len(self.ccols))  # pq's bias slot
    query = property(lambda self: (len(self.dcols) * BINS + len(self.ccols) + 1 + 3) & ~3)  # floats per pq


def _kind(name, code, cols, discrete, continuous, max_rows):
    spec = _sets.SetSpec("embed_logits", "nmh_embed_logits", "sets", "M", name + " rows", name, cols,
                         (len(discrete) * BINS + len(continuous) + 1 + 3) & ~3, max_rows, share=True, kind=code)
    return Kind(name, code, cols, tuple(c for c, _ in discrete), tuple(o for _, o in discrete),
                tuple(c for c, _ in continuous), tuple(s for _, s in continuous), max_rows, spec)


_EXP, _LEVEL = 100, 10
_SKILLS = ("melee", "range", "mage", "fishing", "herbalism", "prospecting", "carving")
# the reference's constructor values (takeru/policy.py:121-161), alchemy's swapped pair included: a
# checkpoint was trained with alchemy_level / 100 and alchemy_exp / 10
_ENTITY_CONT = [("row", 256), ("col", 256), ("damage", 100), ("time_alive", 1024), ("freeze", 3), ("item_level", 50),
                ("latest_combat_tick", 1024), ("gold", 100), ("health", 100), ("food", 100), ("water", 100),
                *[p for s in _SKILLS for p in ((s + "_level", _LEVEL), (s + "_exp", _EXP))],
                ("alchemy_level", _EXP), ("alchemy_exp", _LEVEL)]
ENTITY = _kind("entity", 0, 31,
               [(abi.F[name], 256 * i) for i, name in enumerate(("id", "npc_type", "attacker_id", "message"))],
               [(abi.F[name], s) for name, s in _ENTITY_CONT], 256)
ITEM = _kind("item", 1, 16, [(1, 2), (14, 0)],
             list(zip([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15], [10, 10, 10, 100, 100, 100, 40, 40, 40, 100, 100, 100])),
             1024)
ID_COL = 0


# ---------------------------------------------------------------- plain torch
def embed_features_ref(kind: Kind, sets: torch.Tensor):
    """(idx int64 [..., R, D], cont [..., R, C]) of sets [..., R, cols] in plain torch, any device and
    dtype: SPEC §25's rule, the reference's lines 190-195 / 249-254 with NaN -> 0 where `.long()` is
    undefined. Floating inputs keep their dtype (cont is one division in it), integer inputs give float32."""
    dt = sets.dtype if sets.is_floating_point() else torch.float32
    x = sets.to(dt)
    v = x[..., list(kind.dcols)] + torch.tensor(kind.doffs, dtype=dt, device=x.device)
    idx = torch.where(torch.isnan(v), torch.zeros_like(v), v).clip(0, BINS - 1).long()  # trunc and clip commute here
    cont = x[..., list(kind.ccols)] / torch.tensor(kind.cdivs, dtype=dt, device=x.device)
    return idx, cont


def own_row_ref(ents: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """The index [N] int64 of each row's own entity of ents [N, R, 31]: the first j whose column 0
    equals the row's id and is not 0, else 0 (SPEC §21's rule, the reference's lines 177-182)."""
    col = ents[..., ID_COL]
    return _sets.own_row_index(col if col.is_floating_point() else col.to(torch.float32), ids)


# ---------------------------------------------------------------- the kernels
def _call(kind: Kind, sets, ids, set_rows, want):
    if not sets.is_cuda or (ids is not None and not ids.is_cuda):
        raise HeadsError("embed_features / embed_counts / embed_own run on the GPU: sets and ids must be device tensors")
    x, stride, rows, ek = _sets.set_arg(sets.detach(), set_rows, kind.spec)
    m, dev = x.shape[0], x.device
    idt, id_stride, id_kind = (None, 1, _sets.ELEM_F32) if ids is None else _sets.id_arg(ids.detach(), m)
    D, C = kind.D, kind.C

    def new(name, shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=dev) if name in want else None

    out = dict(idx=new("idx", (m, rows, D), torch.uint8), cont=new("cont", (m, rows, C)),
               counts=new("counts", (m, D, BINS)), sums=new("sums", (m, C)), mine_idx=new("mine_idx", (m,), torch.int32),
               mine_i=new("mine_i", (m, D), torch.uint8), mine_c=new("mine_c", (m, C)))
    with torch.cuda.device(dev):
        heads.check(heads.lib().nmh_embed_features(
            kind.code, m, x.data_ptr(), stride, ek, rows, _ptr(idt), id_stride, id_kind,
            *(_ptr(out[k]) for k in ("idx", "cont", "counts", "sums", "mine_idx", "mine_i", "mine_c")),
            heads._stream()), "nmh_embed_features")
    return out


def embed_features(kind: Kind, sets: torch.Tensor, *, set_rows=None):
    """(idx uint8 [M, R, D], cont float32 [M, R, C]) of sets on the GPU, bit for bit `embed_features_ref`.

    sets: float32 (flat obs) or int16 (native obs), [M, R, cols] or [M, >= cols R] whose first cols R
        columns are the set (R = `set_rows`, by default all whole candidates of the width). A view
        into the obs buffer is read in place, whatever its row stride and alignment, and never written.
    There is no backward: the obs carry no gradient."""
    out = _call(kind, sets, None, set_rows, ("idx", "cont"))
    return out["idx"], out["cont"]


def embed_counts(kind: Kind, sets: torch.Tensor, *, set_rows=None):
    """(counts float32 [M, D, 256], sums float32 [M, C]) without the per-candidate features: how many
    of a set's R candidates have idx_d == i (exact; zero-padded rows count as the reference counts
    them) and each continuous column's raw float32 sum, not divided, in one fixed order."""
    out = _call(kind, sets, None, set_rows, ("counts", "sums"))
    return out["counts"], out["sums"]


def embed_own(ents: torch.Tensor, ids: torch.Tensor, *, set_rows=None):
    """(mine_i uint8 [N, D], mine_c float32 [N, C], mine_idx int32 [N]): each row's own entity by
    `own_row_ref` and its idx and cont. ids: the rows' AgentId, float32 or int16, [N] or [N, 1] with any
    stride: the obs rows' own column is read in place. Only column 0 of the sets is scanned."""
    out = _call(ENTITY, ents, ids, set_rows, ("mine_idx", "mine_i", "mine_c"))
    return out["mine_i"], out["mine_c"], out["mine_idx"]


def embed_logits(kind: Kind, sets: torch.Tensor, pq: torch.Tensor, mask_rows: torch.Tensor, mask_off, *,
                 share: int = 1, mask_kind=None, set_rows=None) -> torch.Tensor:
    """The logits [N, len(mask_off) * (R + 1)] of up to four pointer heads over one set per row, from
    the candidates' own columns (SPEC.md §25): head h's entries are columns [h (R + 1), (h + 1) (R + 1)).

    sets: as for `embed_features`; obs row r reads set r // share.
    pq: float32 [N, heads, kind.query], the encoder's `pointer_query` of the heads' queries.
    mask_rows, mask_off: as for `item.item_logits`.
    A legal candidate's logit is pq[bias] + sum_d pq[256 d + idx_d] + sum_c pq[256 D + c] x_c / s_c in
    that order; an illegal candidate's and the no-op's are 0.0, and a candidate no head allows is never
    read. The backward gives pq's gradient alone, without atomics: the same bits on every run. The
    sets and the mask must not be rewritten between forward and backward."""
    return _sets.SetLogits.apply(kind.spec, sets, pq, mask_rows, tuple(int(o) for o in mask_off), share, mask_kind,
                                 set_rows)


# ---------------------------------------------------------------- the encoders
class _EmbeddedEncoder(nn.Module):
    """What the two encoders share: `embedding` and one linear layer over cat(E[idx], cont)."""

    kind: Kind
    layer: str  # the linear layer's name in the reference

    def __init__(self, table_rows: int, hidden_size: int, fused: bool):
        super().__init__()
        self.fused = bool(fused)
        self.embedding = nn.Embedding(table_rows, EMBED)
        setattr(self, self.layer, nn.Linear(self.kind.features, hidden_size))

    @property
    def _fc(self) -> nn.Linear:
        return getattr(self, self.layer)

    def _sets(self, sets: torch.Tensor, set_rows) -> torch.Tensor:
        return _sets.as_sets(sets, set_rows, self.kind.cols)

    def _feat(self, idx: torch.Tensor, cont: torch.Tensor) -> torch.Tensor:
        """cat(E[idx], cont) [..., 32 D + C]: the reference's lines 191-198."""
        return torch.cat([self.embedding(idx.long()).flatten(-2), cont.to(self.embedding.weight.dtype)], -1)

    def features(self, sets: torch.Tensor, set_rows=None) -> torch.Tensor:
        if self.fused:
            return self._feat(*embed_features(self.kind, sets, set_rows=set_rows))
        return self._feat(*embed_features_ref(self.kind, self._sets(sets, set_rows).to(self.embedding.weight.dtype)))

    def embed(self, sets: torch.Tensor, set_rows=None) -> torch.Tensor:
        """fc(feat) [M, R, H]: the reference's embeddings."""
        return self._fc(self.features(sets, set_rows))

    def pooled(self, sets: torch.Tensor, set_rows=None) -> torch.Tensor:
        """mean_j fc(feat_j) [M, H]. Fused: fc of the mean feature, from the bin counts and column sums."""
        if not self.fused:
            return self.embed(sets, set_rows).mean(1)
        k, rows = self.kind, _sets.set_rows_of(sets, set_rows, self.kind.cols)
        counts, sums = embed_counts(k, sets, set_rows=set_rows)
        mean_e = (counts @ self.embedding.weight[:BINS]).flatten(-2) / rows
        mean_c = sums / torch.tensor(k.cdivs, dtype=sums.dtype, device=sums.device) / rows
        return self._fc(torch.cat([mean_e, mean_c], -1))

    def pointer_query(self, q: torch.Tensor) -> torch.Tensor:
        """pq [N, heads, kind.query] of the heads' queries q [N, heads, H]: the D x 256 scores
        (q W)[32 d, 32 d + 32) . E[i], the C weights (q W)[32 D + c], q . b and zero pads, so that
        q . fc(feat) = pq[bias] + sum_d pq[256 d + idx_d] + sum_c pq[256 D + c] cont_c."""
        k, fc = self.kind, self._fc
        qw = q @ fc.weight
        bins = qw[..., :k.D * EMBED].unflatten(-1, (k.D, EMBED)) @ self.embedding.weight[:BINS].T
        return torch.cat([bins.flatten(-2), qw[..., k.D * EMBED:], (q @ fc.bias).unsqueeze(-1),
                          q.new_zeros(*q.shape[:-1], k.query - k.bias - 1)], -1)


class ReducedPlayerEncoder(_EmbeddedEncoder):
    """The reference's ReducedPlayerEncoder (takeru/policy.py:115-207): `embedding [1024, 32]`,
    `agent_fc = Linear(155, hidden_size)` over every entity's feature and `my_agent_fc = Linear(155,
    input_size)` over the row's own entity's, named as there. Only table rows 0..255 are ever read:
    the clip comes after the offset (SPEC.md §25). Entity sets are [N, R, 31] or [N, >= 31 R] views of
    obs rows (then pass `set_rows`); they are never written.

    `fused=False` is the reference's chain in torch. `fused=True` takes the indices and scaled columns
    (`embed`), the counts and sums (`pooled`) and the own row (`my_agent`) from the HIP kernels."""

    kind, layer = ENTITY, "agent_fc"

    def __init__(self, input_size: int, hidden_size: int, fused: bool = False):
        super().__init__(ENTITY.D * BINS, hidden_size, fused)
        self.my_agent_fc = nn.Linear(ENTITY.features, input_size)

    def my_agent(self, ents: torch.Tensor, ids: torch.Tensor, set_rows=None) -> torch.Tensor:
        """relu(my_agent_fc(feat of the row's own entity)) [N, input_size]: the reference's my_agent."""
        if self.fused:
            mine_i, mine_c, _ = embed_own(ents, ids, set_rows=set_rows)
        else:
            sets = self._sets(ents, set_rows)
            own = sets[torch.arange(sets.shape[0], device=sets.device), own_row_ref(sets, ids)]
            mine_i, mine_c = embed_features_ref(ENTITY, own.to(self.embedding.weight.dtype))
        return F.relu(self.my_agent_fc(self._feat(mine_i, mine_c)))


class ReducedItemEncoder(_EmbeddedEncoder):
    """The reference's ReducedItemEncoder (takeru/policy.py:215-258): `embedding [256, 32]` and
    `fc = Linear(76, hidden_size)`, named as there; `input_size` is unused there too. Item sets are
    [M, R, 16] or [M, >= 16 R] views of obs rows (then pass `set_rows`); they are never written."""

    kind, layer = ITEM, "fc"

    def __init__(self, input_size: int, hidden_size: int, fused: bool = False):
        super().__init__(BINS, hidden_size, fused)
