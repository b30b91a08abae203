"""The reference's player path (baseline_policy.py:43-45, 52, 115-145, 222-230) without its embeddings
(nmh_player_features / nmh_player_logits / nmh_player_logits_backward of libnmmo_heads.so,
include/nmmo_heads.h, SPEC.md §21).

`PlayerEncoder.agent_fc` is linear and its input is a fixed 35-feature function x of an entity's 31
columns (column 0, five npc_type one-hots, columns 2..30 raw), so

    mean_j agent_fc(x_j) = agent_fc(mean_j x_j)        `player_sums`: one [N, 35] sum, then a small linear
    q . agent_fc(x_j)    = (W^T q) . x_j + q . b       `player_logits`: candidate j's own 124 bytes, read in
                                                       place, and only where the mask says j is legal
    my_agent_fc(x_own)                                 `player_own`: x of the one entity whose id is the row's

and neither the [N, 100, H] entity embeddings nor their gradient ever exist: the backward of
`player_logits` is the 36-float sum g_pq = sum_j g_j (x_j, 1).

    enc = PlayerEncoder(64, 64, fused=True).cuda()
    ents = obs[:, o_entity:o_entity + 100 * 31]                    # a view, read in place
    pooled = enc.pooled(ents)                                      # [N, 64]
    mine = enc.my_agent(ents, obs[:, o_agent_id])                  # [N, 64]
    logits = player_logits(ents, enc.pointer_query(q), obs, [mask_off_attack_target])   # [N, 101]

There is no torch fallback for the fused path: a host tensor, or a missing library, is a `HeadsError`.
"""

from __future__ import annotations

import torch
from torch import nn
from torch.nn import functional as F

from . import _sets, heads
from .heads import HeadsError

COLS, FEATURES, TYPES, QUERY = 31, 35, 5, 40
MAX_ROWS, MAX_HEADS = 256, 4
PLAYER_F32, PLAYER_I16 = 0, 1
ID_COL, TYPE_COL = 0, 1


SPEC = _sets.SetSpec("player_logits", "nmh_player_logits", "ents", "N", "entities", "entity", COLS, QUERY, MAX_ROWS,
                     share=False)
NmhPlayerHeads = _sets.NmhSetHeads
_ptr = heads.ptr


def player_heads_struct(mask_off, out_off) -> NmhPlayerHeads:
    return _sets.set_heads_struct(mask_off, out_off, "entity")


def player_features_ref(ents: torch.Tensor) -> torch.Tensor:
    """x [..., R, 35] of entities [..., R, 31] in plain torch, any device and dtype: the reference's
    lines 124-130 with SPEC §21's clamp where `one_hot` would raise (npc_type to 0..4, NaN to 0).
    Floating inputs keep their dtype, integer inputs give float32."""
    dt = ents.dtype if ents.is_floating_point() else torch.float32
    x = ents.to(dt)
    t = torch.nan_to_num(x[..., TYPE_COL], nan=0.0).clip(0, TYPES - 1).long()
    return torch.cat([x[..., :1], F.one_hot(t, TYPES).to(dt), x[..., 2:]], -1)


def own_row_ref(ents: torch.Tensor, ids: torch.Tensor):
    """(x [N, 35] of each row's own entity, its index [N] int64) of entities [N, R, 31] and the rows'
    AgentId [N] in plain torch: the first j whose column 0 equals the id and is not 0, else 0 (the
    reference's lines 132-140). A NaN id matches nothing."""
    feats = player_features_ref(ents)
    idx = _sets.own_row_index(feats[..., ID_COL], ids)
    return feats[torch.arange(feats.shape[0], device=feats.device), idx], idx


def _ent_arg(x: torch.Tensor, set_rows):
    """(tensor kept alive, set stride in elements, R, NMH_PLAYER_*) of entity sets read in place."""
    return _sets.set_arg(x, set_rows, SPEC)


_id_arg = _sets.id_arg


def _features(ents, ids, set_rows, want: str):
    if not ents.is_cuda or (ids is not None and not ids.is_cuda):
        raise HeadsError("player_features / player_sums / player_own run on the GPU: ents and ids must be device "
                         "tensors")
    x, stride, rows, kind = _ent_arg(ents.detach(), set_rows)
    n, dev = x.shape[0], x.device
    idt, id_stride, id_kind = (None, 1, PLAYER_F32) if ids is None else _id_arg(ids.detach(), n)
    f32 = dict(dtype=torch.float32, device=dev)
    feats = torch.empty((n, rows, FEATURES), **f32) if want == "features" else None
    sums = torch.empty((n, FEATURES), **f32) if want == "sums" else None
    mine = torch.empty((n, FEATURES), **f32) if want == "own" else None
    idx = torch.empty((n,), dtype=torch.int32, device=dev) if want == "own" else None
    with torch.cuda.device(dev):
        heads.check(heads.lib().nmh_player_features(
            n, x.data_ptr(), stride, kind, rows, _ptr(idt), id_stride, id_kind, _ptr(feats), _ptr(sums), _ptr(mine),
            _ptr(idx), heads._stream()), "nmh_player_features")
    return feats, sums, mine, idx


def player_features(ents: torch.Tensor, *, set_rows=None) -> torch.Tensor:
    """x [N, R, 35] float32 of entity sets on the GPU (SPEC.md §21), bit for bit `player_features_ref`.

    ents: float32 (flat obs) or int16 (native obs), [N, R, 31] or [N, >= 31 R] whose first 31 R
        columns are the set (R = `set_rows`, by default all whole entities of the width). A view into
        the obs buffer is read in place, whatever its row stride and alignment, and never written.
    There is no backward: the obs carry no gradient."""
    return _features(ents, None, set_rows, "features")[0]


def player_sums(ents: torch.Tensor, *, set_rows=None) -> torch.Tensor:
    """sum_j x_j [N, 35] float32 without the [N, R, 35] features: the class counts exactly, and each
    raw column's float32 sum in one fixed order. Arguments as for `player_features`."""
    return _features(ents, None, set_rows, "sums")[1]


def player_own(ents: torch.Tensor, ids: torch.Tensor, *, set_rows=None):
    """(mine [N, 35] float32, idx [N] int32): each row's own entity, the first j whose column 0 equals
    the row's id and is not 0, else entity 0, and its features x, as `own_row_ref` gives them.

    ents: as for `player_features`. ids: the rows' AgentId, float32 or int16, [N] or [N, 1] with any
        stride: the obs rows' own column is read in place."""
    return _features(ents, ids, set_rows, "own")[2:]


def player_logits(ents: torch.Tensor, pq: torch.Tensor, mask_rows: torch.Tensor, mask_off, *, mask_kind=None,
                  set_rows=None) -> torch.Tensor:
    """The logits [N, len(mask_off) * (R + 1)] of up to four pointer heads over one entity set per
    row, from the entities themselves (SPEC.md §21): head h's entries are columns [h (R + 1), (h + 1) (R + 1)).

    ents: as for `player_features`; obs row r reads set r.
    pq: float32 [N, heads, 40], `PlayerEncoder.pointer_query` of the heads' queries.
    mask_rows: the obs rows themselves (float32, legal iff > 0) or a uint8 / bool mask, [N, >=
        mask_off[h] + R + 1]; mask_off[h] is head h's first entry in a row.
    A legal candidate's logit is pq . (x_j, 1); an illegal candidate's and the no-op's (the
    reference's zero padding row) are 0.0, and an entity no head allows is never read. The
    backward gives pq's gradient alone, without atomics: the same bits on every run. The entities
    and the mask must not be rewritten between forward and backward."""
    return _sets.SetLogits.apply(SPEC, ents, pq, mask_rows, tuple(int(o) for o in mask_off), 1, mask_kind, set_rows)


class PlayerEncoder(nn.Module):
    """The reference's PlayerEncoder (baseline_policy.py:115-145): `agent_fc = Linear(35, hidden_size)`
    over every entity's 35 features and `my_agent_fc = Linear(35, input_size)` over the row's own
    entity's, named as there so a `state_dict` moves both ways. Entity sets are [N, R, 31] or
    [N, >= 31 R] views of obs rows (then pass `set_rows`); they are never written.

    `fused=False` is the reference's chain in torch. `fused=True` takes the features (`embed`), their
    sums (`pooled`) and the own row (`my_agent`) from the HIP kernels, reading the rows in place."""

    def __init__(self, input_size: int, hidden_size: int, fused: bool = False):
        super().__init__()
        self.fused = bool(fused)
        self.agent_fc = nn.Linear(FEATURES, hidden_size)
        self.my_agent_fc = nn.Linear(FEATURES, input_size)

    def features(self, ents: torch.Tensor, set_rows=None) -> torch.Tensor:
        if self.fused:
            return player_features(ents, set_rows=set_rows)
        return player_features_ref(_sets.as_sets(ents, set_rows, COLS)).to(self.agent_fc.weight.dtype)

    def embed(self, ents: torch.Tensor, set_rows=None) -> torch.Tensor:
        """agent_fc(x) [N, R, H]: the reference's agent_embeddings."""
        return self.agent_fc(self.features(ents, set_rows))

    def pooled(self, ents: torch.Tensor, set_rows=None) -> torch.Tensor:
        """mean_j agent_fc(x_j) [N, H]. Fused: agent_fc(sum_j x_j / R), without the [N, R, .] tensors."""
        if self.fused:
            sums = player_sums(ents, set_rows=set_rows)
            return F.linear(sums / _sets.set_rows_of(ents, set_rows, COLS), self.agent_fc.weight, self.agent_fc.bias)
        return self.embed(ents, set_rows).mean(1)

    def my_agent(self, ents: torch.Tensor, ids: torch.Tensor, set_rows=None) -> torch.Tensor:
        """relu(my_agent_fc(x of the row's own entity)) [N, input_size]: the reference's my_agent."""
        if self.fused:
            mine = player_own(ents, ids, set_rows=set_rows)[0]
        else:
            mine = own_row_ref(_sets.as_sets(ents, set_rows, COLS), ids)[0].to(self.my_agent_fc.weight.dtype)
        return F.relu(self.my_agent_fc(mine))

    def pointer_query(self, q: torch.Tensor) -> torch.Tensor:
        """pq [N, heads, 40] of the heads' queries q [N, heads, H]: (q W, q . b, 0, 0, 0, 0), so that
        q . agent_fc(x) = pq[:35] . x + pq[35]."""
        w, b = self.agent_fc.weight, self.agent_fc.bias
        return torch.cat([q @ w, (q @ b).unsqueeze(-1), q.new_zeros(*q.shape[:-1], QUERY - FEATURES - 1)], -1)
