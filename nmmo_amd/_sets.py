"""What `item.py`, `player.py` and `embed.py` share: pointer heads over a candidate set that is read
from the obs rows in place (include/nmmo_heads.h, NmhSetHeads; SPEC.md §20, §21, §25). One C struct,
one argument rule for the sets, one `torch.autograd.Function` over nmh_item_logits / nmh_player_logits /
nmh_embed_logits and their backwards, and the encoders' set reshaping, id argument and own-row rule.
A `SetSpec` holds what differs between the kinds of set.
"""

from __future__ import annotations

import ctypes
from typing import NamedTuple

import torch

from . import heads
from .heads import HeadsError

MAX_HEADS = 4
ELEM_F32, ELEM_I16 = 0, 1


class SetSpec(NamedTuple):
    what: str  # the Python entry point, as messages name it: "item_logits"
    fn: str  # the library's forward, "nmh_item_logits"; its backward is fn + "_backward"
    name: str  # the argument: "items"
    lead: str  # what its messages call the number of sets: "M"
    noun: str  # its elements: "items"
    one: str  # "item"
    cols: int
    query: int  # floats per projected query
    max_rows: int
    share: bool  # whether several obs rows may read one set (the library's `share` argument)
    kind: int | None = None  # the library call's leading `kind` argument (nmh_embed_*), if it has one


class NmhSetHeads(ctypes.Structure):
    _fields_ = [("n_heads", ctypes.c_int32), ("mask_off", ctypes.c_int32 * MAX_HEADS),
                ("out_off", ctypes.c_int32 * MAX_HEADS)]


def set_heads_struct(mask_off, out_off, one: str) -> NmhSetHeads:
    mask_off, out_off = [int(o) for o in mask_off], [int(o) for o in out_off]
    if not 1 <= len(mask_off) <= MAX_HEADS or len(out_off) != len(mask_off):
        raise ValueError(f"between 1 and {MAX_HEADS} heads over one {one} set, got {len(mask_off)}")
    sh = NmhSetHeads()
    sh.n_heads = len(mask_off)
    for h, (m, o) in enumerate(zip(mask_off, out_off)):
        sh.mask_off[h], sh.out_off[h] = m, o
    return sh


def elem_kind(t: torch.Tensor, what: str) -> int:
    if t.dtype == torch.float32:
        return ELEM_F32
    if t.dtype == torch.int16:
        return ELEM_I16
    raise TypeError(f"{what} must be float32 or int16, got {t.dtype}")


def set_arg(x: torch.Tensor, set_rows, spec: SetSpec):
    """(tensor kept alive, set stride in elements, R, NMH_ELEM_*) of candidate sets read in place:
    [M, R, cols], or [M, >= cols R] whose first cols R columns are the set."""
    name, lead, noun, cols, max_rows = spec.name, spec.lead, spec.noun, spec.cols, spec.max_rows
    if x.dim() == 3:
        if x.shape[2] != cols:
            raise ValueError(f"{name} must be [{lead}, R, {cols}] or [{lead}, >= {cols} R], got {tuple(x.shape)}")
        rows = x.shape[1]
        if x.stride(2) != 1 or x.stride(1) != cols:
            x = x.contiguous()
        x = x.as_strided((x.shape[0], rows * cols), (x.stride(0), 1), x.storage_offset())  # the same memory
    elif x.dim() == 2:
        rows = x.shape[1] // cols if set_rows is None else int(set_rows)
    else:
        raise ValueError(f"{name} must be [{lead}, R, {cols}] or [{lead}, >= {cols} R], got {tuple(x.shape)}")
    if set_rows is not None and int(set_rows) != rows:
        raise ValueError(f"set_rows {set_rows} does not match {name} {tuple(x.shape)}")
    if not 1 <= rows <= max_rows or x.shape[1] < rows * cols:
        raise ValueError(f"a set has 1..{max_rows} {noun} of {cols} columns, got {rows} in {tuple(x.shape)}")
    kind = elem_kind(x, name)
    x, stride = heads.rows_arg(x, rows * cols)
    return x, stride, rows, kind


def set_rows_of(x: torch.Tensor, set_rows, cols: int) -> int:
    """R of sets [M, R, cols] or [M, >= cols R]: by default all whole candidates of the width."""
    return x.shape[1] if x.dim() == 3 else (x.shape[1] // cols if set_rows is None else int(set_rows))


def as_sets(x: torch.Tensor, set_rows, cols: int) -> torch.Tensor:
    """[M, R, cols] of sets [M, R, cols] or [M, >= cols R], for the plain-torch paths."""
    if x.dim() == 3:
        return x
    rows = set_rows_of(x, set_rows, cols)
    return x[:, :rows * cols].reshape(x.shape[0], rows, cols)


def id_arg(ids: torch.Tensor, n: int):
    """(tensor kept alive, element stride, NMH_ELEM_*) of the rows' AgentId read in place: [N] or
    [N, 1], any positive stride (a column of the obs rows)."""
    if ids.dim() == 2 and ids.shape[1] == 1:
        ids = ids[:, 0]
    if ids.dim() != 1 or ids.shape[0] != n:
        raise ValueError(f"ids must be [{n}] or [{n}, 1], got {tuple(ids.shape)}")
    kind = elem_kind(ids, "ids")
    if n > 1 and ids.stride(0) < 1:
        ids = ids.contiguous()
    return ids, max(ids.stride(0), 1), kind


def own_row_index(col: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """The index [N] int64 of each row's own entity from the entities' id column [N, R] (floating) and
    the rows' AgentId: the first j whose id equals the row's and is not 0, else 0 (SPEC §21's rule). A
    NaN id matches nothing."""
    match = (col == ids.reshape(-1, 1).to(col.dtype)) & (col != 0)
    return torch.where(match.any(1), match.int().argmax(1), torch.zeros_like(match.sum(1)))


class SetLogits(torch.autograd.Function):
    """`item_logits`, `player_logits` and `embed_logits`: the logits of up to four pointer heads over
    one set per row."""

    @staticmethod
    def forward(ctx, spec, sets, pq, mask_rows, mask_off, share, mask_kind, set_rows):
        what, fn, name, one, query, shared = spec.what, spec.fn, spec.name, spec.one, spec.query, spec.share
        if not (sets.is_cuda and pq.is_cuda and mask_rows.is_cuda):
            raise HeadsError(f"{what} runs on the GPU: {name}, pq and mask_rows must be device tensors")
        x, stride, rows, kind = set_arg(sets.detach(), set_rows, spec)
        n_heads = len(mask_off)
        n, dev = mask_rows.shape[0], x.device
        if pq.dtype != torch.float32 or tuple(pq.shape) != (n, n_heads, query):
            raise ValueError(f"pq must be float32 [{n}, {n_heads}, {query}], got {pq.dtype} {tuple(pq.shape)}")
        if shared:
            share = int(share)
            if share < 1 or x.shape[0] * share < n:
                raise ValueError(f"{x.shape[0]} {one} sets shared by {share} rows each do not cover {n} rows")
        elif x.shape[0] != n:
            raise ValueError(f"{x.shape[0]} {one} sets for {n} rows")
        width = rows + 1
        sh = set_heads_struct(mask_off, [h * width for h in range(n_heads)], one)
        mask, mptr, mstride, mkind = heads._mask_arg(mask_rows, n, max(int(o) for o in mask_off) + width)
        if mask_kind is not None and mask_kind != mkind:
            raise ValueError(f"mask_kind {mask_kind} does not match the mask's dtype {mask_rows.dtype}")
        pq = heads._dense16(pq)
        out = torch.empty((n, n_heads * width), dtype=torch.float32, device=dev)
        # the set's arguments up to the mask: the library's entity entry points take no `share`
        head = (ctypes.byref(sh), n, x.data_ptr(), stride, kind, rows)
        if spec.kind is not None:
            head = (spec.kind,) + head
        if shared:
            head += (share,)
        with torch.cuda.device(dev):
            heads.check(getattr(heads.lib(), fn)(*head, mptr, mstride, mkind, pq.data_ptr(), out.data_ptr(),
                                                 n_heads * width, heads._stream()), fn)
        ctx.args = (spec, head, rows, mstride, mkind, n_heads)  # (head keeps sh alive; save_for_backward keeps x)
        ctx.save_for_backward(x, mask)
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, mask = ctx.saved_tensors
        spec, head, rows, mstride, mkind, n_heads = ctx.args
        n, dev = mask.shape[0], x.device
        g_out = g_out.to(torch.float32).contiguous()
        g_pq = torch.empty((n, n_heads, spec.query), dtype=torch.float32, device=dev)  # (n == 0: empty, nothing to write)
        with torch.cuda.device(dev):
            heads.check(getattr(heads.lib(), spec.fn + "_backward")(
                *head, mask.data_ptr(), mstride, mkind, g_out.data_ptr(), n_heads * (rows + 1), g_pq.data_ptr(),
                heads._stream()), spec.fn + "_backward")
        return None, None, g_pq, None, None, None, None, None
