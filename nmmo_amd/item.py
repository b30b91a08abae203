"""The reference's item path (baseline_policy.py:47-51, 148-190, 222-230) without its embeddings
(nmh_item_features / nmh_item_logits / nmh_item_logits_backward of libnmmo_heads.so,
include/nmmo_heads.h, SPEC.md §20).

`ItemEncoder.fc` is linear and its input is a fixed 32-feature function x of an item's 16 columns
(18 type one-hots, 2 equipped one-hots, 12 columns scaled by 0.01), so

    mean_j fc(x_j) = fc(mean_j x_j)              `item_sums`: one [M, 32] sum, then a small linear
    q . fc(x_j)    = (W^T q) . x_j + q . b       `item_logits`: candidate j's own 64 bytes, read in
                                                 place, and only where the mask says j is legal

and neither the [N, 1024, H] market embeddings nor their gradient ever exist: the backward of
`item_logits` is the 33-float sum g_pq = sum_j g_j (x_j, 1).

    enc = ItemEncoder(64, fused=True).cuda()
    market = obs[:, o_market:o_market + 1024 * 16]                 # a view, read in place
    pooled = enc.pooled(market)                                    # [N, 64]
    logits = item_logits(market, enc.pointer_query(q), obs, [mask_off_buy])   # [N, 1025]

There is no torch fallback for the fused path: a host tensor, or a missing library, is a `HeadsError`.
"""

from __future__ import annotations

import torch
from torch import nn
from torch.nn import functional as F

from . import _sets, heads
from .heads import HeadsError

COLS, FEATURES, TYPES, QUERY = 16, 32, 18, 36
MAX_ROWS, MAX_HEADS = 1024, 4
ITEM_F32, ITEM_I16 = 0, 1
TYPE_COL, EQUIPPED_COL = 1, 14
CONT_COLS = [3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15]
SCALE = 0.01  # applied as the float32 nearest 0.01, the reference's `continuous_scale`


SPEC = _sets.SetSpec("item_logits", "nmh_item_logits", "items", "M", "items", "item", COLS, QUERY, MAX_ROWS, share=True)
NmhItemHeads = _sets.NmhSetHeads


def item_heads_struct(mask_off, out_off) -> NmhItemHeads:
    return _sets.set_heads_struct(mask_off, out_off, "item")


def item_features_ref(items: torch.Tensor) -> torch.Tensor:
    """x [..., R, 32] of items [..., R, 16] in plain torch, any device and dtype: the reference's
    lines 162-168 with SPEC §20's clamps where `one_hot` would raise (type to 0..17, equipped to
    0..1, NaN to 0). Floating inputs keep their dtype, integer inputs give float32."""
    dt = items.dtype if items.is_floating_point() else torch.float32
    x = items.to(dt)
    cls = torch.nan_to_num(x[..., [TYPE_COL, EQUIPPED_COL]], nan=0.0)
    t = cls[..., 0].clip(0, TYPES - 1).long()
    e = cls[..., 1].clip(0, 1).long()
    scale = torch.tensor(SCALE, dtype=torch.float32, device=items.device).to(dt)
    return torch.cat([F.one_hot(t, TYPES).to(dt), F.one_hot(e, 2).to(dt), x[..., CONT_COLS] * scale], -1)


def _item_arg(x: torch.Tensor, set_rows):
    """(tensor kept alive, set stride in elements, R, NMH_ITEM_*) of item sets read in place."""
    return _sets.set_arg(x, set_rows, SPEC)


def _features(items, set_rows, want_features: bool, want_sums: bool):
    if not items.is_cuda:
        raise HeadsError("item_features / item_sums run on the GPU: items must be a device tensor")
    x, stride, rows, kind = _item_arg(items.detach(), set_rows)
    m, dev = x.shape[0], x.device
    feats = torch.empty((m, rows, FEATURES), dtype=torch.float32, device=dev) if want_features else None
    sums = torch.empty((m, FEATURES), dtype=torch.float32, device=dev) if want_sums else None
    with torch.cuda.device(dev):
        heads.check(heads.lib().nmh_item_features(
            m, x.data_ptr(), stride, kind, rows, None if feats is None else feats.data_ptr(),
            None if sums is None else sums.data_ptr(), heads._stream()), "nmh_item_features")
    return feats, sums


def item_features(items: torch.Tensor, *, set_rows=None) -> torch.Tensor:
    """x [M, R, 32] float32 of item sets on the GPU (SPEC.md §20), bit for bit `item_features_ref`.

    items: float32 (flat obs) or int16 (native obs), [M, R, 16] or [M, >= 16 R] whose first 16 R
        columns are the set (R = `set_rows`, by default all whole items of the width). A view into
        the obs buffer is read in place, whatever its row stride and alignment, and never written.
    There is no backward: the obs carry no gradient."""
    return _features(items, set_rows, True, False)[0]


def item_sums(items: torch.Tensor, *, set_rows=None) -> torch.Tensor:
    """sum_j x_j [M, 32] float32 without the [M, R, 32] features: the class counts exactly, and each
    scaled column as (the sum of the raw column) * 0.01f. Arguments as for `item_features`."""
    return _features(items, set_rows, False, True)[1]


def item_logits(items: torch.Tensor, pq: torch.Tensor, mask_rows: torch.Tensor, mask_off, *, share: int = 1,
                mask_kind=None, set_rows=None) -> torch.Tensor:
    """The logits [N, len(mask_off) * (R + 1)] of up to four pointer heads over one item set per
    row, from the items themselves (SPEC.md §20): head h's entries are columns [h (R + 1), (h + 1) (R + 1)).

    items: as for `item_features`; obs row r reads set r // share (share = 1 for flat rows, the
        players per env for the native per-env Market).
    pq: float32 [N, heads, 36], `ItemEncoder.pointer_query` of the heads' queries.
    mask_rows: the obs rows themselves (float32, legal iff > 0) or a uint8 / bool mask, [N, >=
        mask_off[h] + R + 1]; mask_off[h] is head h's first entry in a row.
    A legal candidate's logit is pq . (x_j, 1); an illegal candidate's and the no-op's (the
    reference's zero padding row) are 0.0, and illegal candidates' items are never read. The
    backward gives pq's gradient alone, without atomics: the same bits on every run. The items
    and the mask must not be rewritten between forward and backward."""
    return _sets.SetLogits.apply(SPEC, items, pq, mask_rows, tuple(int(o) for o in mask_off), share, mask_kind, set_rows)


class ItemEncoder(nn.Module):
    """The reference's ItemEncoder (baseline_policy.py:148-170): `fc = Linear(32, hidden)` over the
    32 item features, named as there so a `state_dict` moves both ways. Item sets are [M, R, 16] or
    [M, >= 16 R] views of obs rows (then pass `set_rows`); they are never written.

    `fused=False` is the reference's chain in torch. `fused=True` takes the features (`embed`) and
    their sums (`pooled`) from the HIP kernels, reading the rows in place."""

    def __init__(self, hidden: int, fused: bool = False):
        super().__init__()
        self.fused = bool(fused)
        self.fc = nn.Linear(FEATURES, hidden)

    def features(self, items: torch.Tensor, set_rows=None) -> torch.Tensor:
        if self.fused:
            return item_features(items, set_rows=set_rows)
        return item_features_ref(_sets.as_sets(items, set_rows, COLS)).to(self.fc.weight.dtype)

    def embed(self, items: torch.Tensor, set_rows=None) -> torch.Tensor:
        """fc(x) [M, R, H]: the reference's forward."""
        return self.fc(self.features(items, set_rows))

    def pooled(self, items: torch.Tensor, set_rows=None) -> torch.Tensor:
        """mean_j fc(x_j) [M, H]. Fused: fc(sum_j x_j / R), without the [M, R, .] tensors."""
        if self.fused:
            rows = _sets.set_rows_of(items, set_rows, COLS)
            return F.linear(item_sums(items, set_rows=set_rows) / rows, self.fc.weight, self.fc.bias)
        return self.embed(items, set_rows).mean(1)

    def pointer_query(self, q: torch.Tensor) -> torch.Tensor:
        """pq [N, heads, 36] of the heads' queries q [N, heads, H]: (q W, q . b, 0, 0, 0), so that
        q . fc(x) = pq[:32] . x + pq[32]."""
        return torch.cat([q @ self.fc.weight, (q @ self.fc.bias).unsqueeze(-1), q.new_zeros(*q.shape[:-1], 3)], -1)
