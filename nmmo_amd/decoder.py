"""All action heads of the start-kit Baseline's decoder in one kernel, reading the obs rows in place
(nmh_decoder_forward / nmh_decoder_backward of libnmmo_heads.so, include/nmmo_heads.h, SPEC.md §23).

    sets = [obs[:, o_entity:o_entity + 100 * 31], obs[:, o_inv:o_inv + 12 * 16], obs[:, o_market:o_market + 1024 * 16]]
    action, logprob, entropy = decoder_heads(dense, pq, [(sets[0], "entity"), (sets[1], "item"), (sets[2], "item")],
                                             head_set, obs, dims)

is `masked_heads(cat(dense heads, item_logits, player_logits))` bit for bit, without the [N, 1586]
logits, their gradient, and the three passes over the mask: a pointer head's logits go from the
candidates' own columns into the LDS tile the masked categorical reads. There is no torch fallback:
a host tensor, or a missing library, is a `HeadsError`.
"""

from __future__ import annotations

import ctypes

import torch

from . import heads, item, player
from .heads import HeadsError

SET_ENTITY, SET_ITEM = 0, 1
ELEM_F32, ELEM_I16 = 0, 1
QUERY = 40  # floats per pointer head in pq: an item head uses 0..32, an entity head 0..35
RULES = {"entity": SET_ENTITY, "item": SET_ITEM, SET_ENTITY: SET_ENTITY, SET_ITEM: SET_ITEM}
COLS = {SET_ENTITY: player.COLS, SET_ITEM: item.COLS}
MAX_ROWS = {SET_ENTITY: player.MAX_ROWS, SET_ITEM: item.MAX_ROWS}


class NmhDecoderSets(ctypes.Structure):
    _fields_ = [("n_sets", ctypes.c_int32), ("elem_kind", ctypes.c_int32), ("rule", ctypes.c_int32 * heads.MAX_SETS),
                ("set_rows", ctypes.c_int32 * heads.MAX_SETS), ("share", ctypes.c_int32 * heads.MAX_SETS),
                ("head_set", ctypes.c_int32 * heads.MAX_HEADS), ("stride", ctypes.c_int64 * heads.MAX_SETS),
                ("base", ctypes.c_void_p * heads.MAX_SETS)]


def sets_struct(head_set, rules, set_rows, shares, strides, bases, elem_kind) -> NmhDecoderSets:
    """The C struct of a call's candidate sets; the rules themselves are checked by the library."""
    if len(rules) > heads.MAX_SETS:
        raise ValueError(f"at most {heads.MAX_SETS} candidate sets, got {len(rules)}")
    if len(head_set) > heads.MAX_HEADS:
        raise ValueError(f"at most {heads.MAX_HEADS} heads, got {len(head_set)}")
    st = NmhDecoderSets()
    st.n_sets, st.elem_kind = len(rules), int(elem_kind)
    for s in range(len(rules)):
        st.rule[s], st.set_rows[s], st.share[s] = int(rules[s]), int(set_rows[s]), int(shares[s])
        st.stride[s], st.base[s] = int(strides[s]), bases[s]
    for k, s in enumerate(head_set):
        st.head_set[k] = int(s)
    return st


def _split_sets(sets, dims, head_set):
    """[(tensor, rule, share, rows)] of the `sets` argument: a tensor ([M, R, 16] items or [M, R, 31]
    entities), or (tensor, rule) / (tensor, rule, share) with rule "item" or "entity"."""
    out = []
    for s, entry in enumerate(sets):
        t, rule, share = (entry, None, 1) if torch.is_tensor(entry) else (tuple(entry) + (1,))[:3]
        if rule is None:
            if t.dim() != 3 or t.shape[2] not in (item.COLS, player.COLS):
                raise ValueError(f"sets[{s}]: pass (tensor, 'item' | 'entity') for a set that is not [M, R, 16 | 31]")
            rule = SET_ITEM if t.shape[2] == item.COLS else SET_ENTITY
        if rule not in RULES:
            raise ValueError(f"sets[{s}]: unknown rule {rule!r}")
        users = [int(dims[k]) - 1 for k, hs in enumerate(head_set) if hs == s]
        if not users:
            raise ValueError(f"no head uses set {s} (head_set)")
        out.append((t, RULES[rule], int(share), users[0]))
    return out


def _make_function():
    class DecoderHeads(torch.autograd.Function):
        @staticmethod
        def forward(ctx, dense, pq, mask, dims, head_set, action, seed, offset, row_base, meta, *set_tensors):
            # the selection mode, a bool, is the last argument where one is given (after the set tensors)
            greedy = bool(set_tensors) and isinstance(set_tensors[-1], bool) and set_tensors[-1]
            set_tensors = [t for t in set_tensors if not isinstance(t, bool)]
            hd = heads.heads_struct(dims)
            dims, head_set = [int(d) for d in dims], [int(s) for s in head_set]
            if len(head_set) != len(dims):
                raise ValueError(f"head_set has {len(head_set)} entries for {len(dims)} heads")
            total, n_ptr = sum(dims), sum(s >= 0 for s in head_set)
            n_dense = sum(d for d, s in zip(dims, head_set) if s < 0)
            tensors = [t for t in (dense, pq, mask, *set_tensors) if t is not None]
            if not all(t.is_cuda for t in tensors):
                raise HeadsError("decoder_heads runs on the GPU: every input must be a device tensor")
            n, dev = mask.shape[0], mask.device
            kept, rules, rows, shares, strides, kinds = [], [], [], [], [], []
            for s, (t, (rule, share, r)) in enumerate(zip(set_tensors, meta)):
                arg = item._item_arg if rule == SET_ITEM else player._ent_arg
                x, stride, r, kind = arg(t.detach(), r if t.dim() == 2 else None)
                if x.data_ptr() != t.data_ptr():
                    raise ValueError(f"sets[{s}] {tuple(t.shape)} with strides {t.stride()} cannot be read in place")
                if share < 1 or x.shape[0] * share < n:
                    raise ValueError(f"sets[{s}]: {x.shape[0]} sets shared by {share} rows each do not cover {n} rows")
                kept.append(x), rules.append(rule), rows.append(r), shares.append(share), strides.append(stride)
                kinds.append(kind)
            if len(set(kinds)) > 1:
                raise TypeError("every candidate set of a call has one element type, float32 or int16")
            if n_ptr:
                if pq is None or pq.dtype != torch.float32 or tuple(pq.shape) != (n, n_ptr, QUERY):
                    raise ValueError(f"pq must be float32 [{n}, {n_ptr}, {QUERY}], got "
                                     f"{None if pq is None else (pq.dtype, tuple(pq.shape))}")
                pq = heads._dense16(pq)
            else:
                pq = None
            d_stride = n_dense
            if n_dense:
                if dense is None or dense.dtype != torch.float32 or tuple(dense.shape) != (n, n_dense):
                    raise ValueError(f"dense must be float32 [{n}, {n_dense}], got "
                                     f"{None if dense is None else (dense.dtype, tuple(dense.shape))}")
                dense, d_stride = heads.rows_arg(dense.detach(), n_dense)
            else:
                dense = None
            st = sets_struct(head_set, rules, rows, shares, strides, [x.data_ptr() for x in kept],
                             kinds[0] if kinds else ELEM_F32)
            mask, mptr, mstride, mkind = heads._mask_arg(mask, n, total)
            a_in, (a_out, logprob, entropy, lse, hent), io = heads.head_io(action, n, hd.n_heads, dev, seed, offset,
                                                                          row_base)
            with torch.cuda.device(dev):
                heads.forward_call("nmh_decoder_forward", greedy,
                                   (ctypes.byref(hd), ctypes.byref(st), n, heads.ptr(pq), heads.ptr(dense), d_stride,
                                    mptr, mstride, mkind), io)
            ctx.args = (hd, st, mstride, mkind, d_stride, n_dense, n_ptr)
            ctx.has = (dense is not None, pq is not None)
            ctx.set_materialize_grads(False)  # an unused logprob / entropy arrives as None -> NULL
            ctx.save_for_backward(mask, a_out, lse, hent, *[t for t in (dense, pq) if t is not None], *kept)
            ctx.mark_non_differentiable(a_out, lse, hent)
            return a_out, logprob, entropy, lse, hent

        @staticmethod
        def backward(ctx, _ga, g_logprob, g_entropy, _gl, _gh):
            mask, actions, lse, hent, *rest = ctx.saved_tensors
            dense = rest.pop(0) if ctx.has[0] else None
            pq = rest.pop(0) if ctx.has[1] else None
            hd, st, mstride, mkind, d_stride, n_dense, n_ptr = ctx.args
            n, dev = mask.shape[0], mask.device
            need = ctx.needs_input_grad  # a gradient nobody asked for is a NULL pointer: not computed
            g_d = torch.empty((n, n_dense), dtype=torch.float32, device=dev) if dense is not None and need[0] else None
            g_q = torch.empty((n, n_ptr, QUERY), dtype=torch.float32, device=dev) if pq is not None and need[1] else None
            glp = None if g_logprob is None else g_logprob.to(torch.float32).contiguous()
            gen = None if g_entropy is None else g_entropy.to(torch.float32).contiguous()
            ptr = heads.ptr
            with torch.cuda.device(dev):
                heads.check(heads.lib().nmh_decoder_backward(
                    ctypes.byref(hd), ctypes.byref(st), n, ptr(pq), ptr(dense), d_stride, mask.data_ptr(), mstride,
                    mkind, actions.data_ptr(), lse.data_ptr(), hent.data_ptr(), ptr(glp), ptr(gen), ptr(g_d), n_dense,
                    ptr(g_q), heads._stream()), "nmh_decoder_backward")
            return (g_d, g_q, *[None] * (len(need) - 2))  # the sets, and the mode where it was passed

    return DecoderHeads


_function = None


def decoder_heads_full(dense, pq, sets, head_set, mask, dims, action=None, *, seed: int = 0, offset: int = 0,
                       row_base: int = 0, greedy: bool = False):
    """`decoder_heads` plus the per-head saved values: (action, logprob, entropy, lse [N, H],
    head_entropy [N, H])."""
    global _function
    heads.check_greedy(greedy, action)
    if _function is None:
        _function = _make_function()
    split = _split_sets(sets, dims, head_set)
    a, logprob, entropy, lse, hent = _function.apply(
        dense, pq, mask, tuple(dims), tuple(head_set), action, seed, offset, row_base,
        tuple((rule, share, rows) for _, rule, share, rows in split), *[t for t, _, _, _ in split], bool(greedy))
    return (a if action is None else action), logprob, entropy, lse, hent


def decoder_heads(dense, pq, sets, head_set, mask, dims, action=None, *, seed: int = 0, offset: int = 0,
                  row_base: int = 0, greedy: bool = False):
    """Every masked categorical head of a batch of obs rows in one kernel, the pointer heads' logits
    taken from the candidates' own columns (SPEC.md §23).

    dims, head_set: per head its size and -1 (dense: its logits are given) or the index s of the
        candidate set it points into; then dims[k] == R_s + 1, the last entry being the no-op with
        logit 0.
    dense: float32 [N, sum of the dense heads' dims] in head order, or None.
    pq: float32 [N, P, 40], one slot per pointer head in head order: `ItemEncoder.pointer_query`
        (36 floats) or `PlayerEncoder.pointer_query` (40) of the head's query, padded to 40.
    sets: per set a view of the obs rows, float32 (flat) or int16 (native), all of one type:
        [M, R, 16] items or [M, R, 31] entities, or (tensor, "item" | "entity"[, share]) for a
        [M, >= cols R] view; obs row r reads set r // share. A set is read in place through its own
        pointer and stride and never copied or written; candidates that a head's mask forbids are
        never addressed.
    mask, action, seed, offset, row_base, greedy: as for `masked_heads`.
    Returns (action, logprob [N], entropy [N]), bit for bit what `masked_heads` returns on the
    logits `item_logits` / `player_logits` would make. logprob and entropy are differentiable with
    respect to dense and pq; a gradient nothing requires is not computed. A call allocates its
    outputs and nothing else. The sets and the mask must not be rewritten between forward and
    backward."""
    return decoder_heads_full(dense, pq, sets, head_set, mask, dims, action, seed=seed, offset=offset,
                              row_base=row_base, greedy=greedy)[:3]
