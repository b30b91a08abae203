"""Fused masked action heads: loader for libnmmo_heads.so and `masked_heads`, the
`torch.autograd.Function` over nmh_forward / nmh_backward (include/nmmo_heads.h, SPEC.md §15).

    action, logprob, entropy = masked_heads(logits, obs, dims)            # sample
    _, logprob, entropy = masked_heads(logits, obs, dims, action=action)  # evaluate, differentiable
    action, logprob, entropy = masked_heads(logits, obs, dims, greedy=True)  # select the argmax (SPEC.md §24)

replaces the per-head `masked_fill(mask == 0, -1e9)` + `Categorical` loop of the reference's
policies (baseline_policy.py:245-262) by one kernel forward and one backward. `pointer_heads`
(nmh_pointer_forward / nmh_pointer_backward, SPEC.md §18) also computes the logits of the
reference's pointer heads, query . key over the row's candidates, inside that kernel. There is no
torch fallback: a missing or stale library is an error.

torch is imported first so that the library binds to the HIP runtime torch loaded (see
`_loader.py`): tensors' device pointers and torch's streams are then valid inside the library.
"""

from __future__ import annotations

import ctypes
import os

from . import _loader, build

LIB_PATH = os.environ.get("NMMO_HEADS_LIB", build.lib_path("heads"))
SYMBOLS = ["nmh_forward", "nmh_backward", "nmh_pointer_forward", "nmh_pointer_backward", "nmh_tile_forward",
           "nmh_tile_backward", "nmh_tile2_forward", "nmh_tile2_backward", "nmh_item_features", "nmh_item_logits",
           "nmh_item_logits_backward", "nmh_player_features", "nmh_player_logits", "nmh_player_logits_backward",
           "nmh_decoder_forward", "nmh_decoder_backward", "nmh_forward_argmax", "nmh_pointer_forward_argmax",
           "nmh_decoder_forward_argmax", "nmh_embed_features", "nmh_embed_logits", "nmh_embed_logits_backward",
           "nmh_last_error", "nmh_build_info"]
MAX_HEADS, MAX_DIM = 16, 2048
MAX_SETS, MAX_KEY_DIM = 4, 256
MASK_F32, MASK_U8 = 0, 1
NMH_OK, NMH_E_INVALID, NMH_E_HIP = 0, -1, -2
_lib = None


class HeadsError(RuntimeError):
    pass


class NmhHeads(ctypes.Structure):
    _fields_ = [("n_heads", ctypes.c_int32), ("dims", ctypes.c_int32 * MAX_HEADS)]


class NmhPointer(ctypes.Structure):
    _fields_ = [("n_sets", ctypes.c_int32), ("key_dim", ctypes.c_int32), ("set_rows", ctypes.c_int32 * MAX_SETS),
                ("head_set", ctypes.c_int32 * MAX_HEADS)]


def declare(L):
    vp, i32, i64, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
    hp, pp, kp = ctypes.POINTER(NmhHeads), ctypes.POINTER(NmhPointer), ctypes.POINTER(ctypes.c_void_p)
    L.nmh_pointer_forward.argtypes = [hp, pp, i32, vp, kp, vp, i64, vp, i64, i32, vp, u64, u64, ctypes.c_uint32,
                                      vp, vp, vp, vp, vp, vp]
    L.nmh_pointer_backward.argtypes = [hp, pp, i32, vp, kp, vp, i64, vp, i64, i32, vp, vp, vp, vp, vp, vp, i64, vp,
                                       kp, vp]
    L.nmh_forward.argtypes = [hp, i32, vp, i64, vp, i64, i32, vp, u64, u64, ctypes.c_uint32, vp, vp, vp, vp, vp, vp]
    L.nmh_backward.argtypes = [hp, i32, vp, i64, vp, i64, i32, vp, vp, vp, vp, vp, vp, i64, vp]
    L.nmh_tile_forward.argtypes = [i32, vp, i64, i32, vp, vp, vp, vp, vp]  # nmmo_amd/tile.py
    L.nmh_tile_backward.argtypes = [i32, vp, vp, vp, i32, vp, vp, vp]
    L.nmh_tile2_forward.argtypes = [i32, vp, i64, i32, vp, vp, vp, vp, vp, vp, vp]
    L.nmh_tile2_backward.argtypes = [i32, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.nmh_item_features.argtypes = [i32, vp, i64, i32, i32, vp, vp, vp]  # nmmo_amd/item.py
    L.nmh_item_logits.argtypes = [vp, i32, vp, i64, i32, i32, i32, vp, i64, i32, vp, vp, i64, vp]
    L.nmh_item_logits_backward.argtypes = [vp, i32, vp, i64, i32, i32, i32, vp, i64, i32, vp, i64, vp, vp]
    L.nmh_player_features.argtypes = [i32, vp, i64, i32, i32, vp, i64, i32, vp, vp, vp, vp, vp]  # nmmo_amd/player.py
    L.nmh_player_logits.argtypes = [vp, i32, vp, i64, i32, i32, vp, i64, i32, vp, vp, i64, vp]
    L.nmh_player_logits_backward.argtypes = [vp, i32, vp, i64, i32, i32, vp, i64, i32, vp, i64, vp, vp]
    # nmmo_amd/embed.py: the kind first, then the set arguments of the item calls
    L.nmh_embed_features.argtypes = [i32, i32, vp, i64, i32, i32, vp, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.nmh_embed_logits.argtypes = [i32] + L.nmh_item_logits.argtypes
    L.nmh_embed_logits_backward.argtypes = [i32] + L.nmh_item_logits_backward.argtypes
    L.nmh_decoder_forward.argtypes = [hp, vp, i32, vp, vp, i64, vp, i64, i32, vp, u64, u64, ctypes.c_uint32,
                                      vp, vp, vp, vp, vp, vp]  # nmmo_amd/decoder.py
    L.nmh_decoder_backward.argtypes = [hp, vp, i32, vp, vp, i64, vp, i64, i32, vp, vp, vp, vp, vp, vp, i64, vp, vp]
    # greedy selection (SPEC.md §24): the forwards without actions_in, seed, offset and row_base
    L.nmh_forward_argmax.argtypes = [hp, i32, vp, i64, vp, i64, i32, vp, vp, vp, vp, vp, vp]
    L.nmh_pointer_forward_argmax.argtypes = [hp, pp, i32, vp, kp, vp, i64, vp, i64, i32, vp, vp, vp, vp, vp, vp]
    L.nmh_decoder_forward_argmax.argtypes = [hp, vp, i32, vp, vp, i64, vp, i64, i32, vp, vp, vp, vp, vp, vp]


def lib():
    global _lib
    if _lib is None:
        _lib = _loader.load("heads", LIB_PATH, HeadsError, "nmh", declare,
                            "there is no torch fallback for the fused heads")
    return _lib


def check(rc: int, what: str):
    if rc != NMH_OK:
        raise HeadsError(f"{what} failed ({rc}): {lib().nmh_last_error().decode()}")


def heads_struct(dims) -> NmhHeads:
    dims = [int(d) for d in dims]
    if not 1 <= len(dims) <= MAX_HEADS:
        raise ValueError(f"between 1 and {MAX_HEADS} heads, got {len(dims)}")
    hd = NmhHeads()
    hd.n_heads = len(dims)
    for k, d in enumerate(dims):
        hd.dims[k] = d
    return hd


def rows_arg(t, width: int):
    """(tensor kept alive, row stride in elements) of t [n, >= width] whose rows' first `width` columns
    the library reads in place: copied only if its columns are not consecutive or its rows overlap."""
    s0, s1 = t.stride()
    if s1 != 1 or (s0 < width and t.shape[0] > 1):
        t = t[:, :width].contiguous()
        s0 = t.stride(0)
    return t, (s0 if s0 > width else width)


def _mask_arg(mask, n_rows: int, total: int):
    """(tensor kept alive, data_ptr, row stride in elements, NMH_MASK_*) of a mask read in place."""
    import torch

    if mask.dim() != 2 or mask.shape[0] != n_rows or mask.shape[1] < total:
        raise ValueError(f"mask must be [{n_rows}, >= {total}], got {tuple(mask.shape)}")
    if mask.dtype == torch.float32:
        kind = MASK_F32
    elif mask.dtype in (torch.uint8, torch.bool):
        kind = MASK_U8
    else:
        raise TypeError(f"mask must be float32, uint8 or bool, got {mask.dtype}")
    mask, stride = rows_arg(mask, total)
    return mask, mask.data_ptr(), stride, kind


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def head_io(action, n: int, n_heads: int, dev, seed, offset, row_base):
    """What every forward of the masked heads passes after its logits and mask: the actions to
    evaluate (None: sample), the philox counter, and the five outputs, which it allocates. Returns
    (a_in kept alive, (a_out, logprob, entropy, lse, hent), the arguments actions_in .. head_entropy)."""
    import torch

    a_in = None
    if action is not None:
        if tuple(action.shape) != (n, n_heads):
            raise ValueError(f"action must be [{n}, {n_heads}], got {tuple(action.shape)}")
        a_in = action.to(device=dev, dtype=torch.int32).contiguous()
    a_out = torch.empty((n, n_heads), dtype=torch.int32, device=dev)
    logprob = torch.empty(n, dtype=torch.float32, device=dev)
    entropy = torch.empty(n, dtype=torch.float32, device=dev)
    lse = torch.empty((n, n_heads), dtype=torch.float32, device=dev)
    hent = torch.empty((n, n_heads), dtype=torch.float32, device=dev)
    return a_in, (a_out, logprob, entropy, lse, hent), (
        None if a_in is None else a_in.data_ptr(), int(seed) & (2**64 - 1), int(offset) & (2**64 - 1),
        int(row_base) & 0xFFFFFFFF, a_out.data_ptr(), logprob.data_ptr(), entropy.data_ptr(), lse.data_ptr(),
        hent.data_ptr())


def check_greedy(greedy: bool, action):
    if greedy and action is not None:
        raise ValueError("greedy=True selects the actions: it cannot be combined with action=")


def forward_call(name: str, greedy: bool, args, io):
    """The forward `name` on the current stream, or with `greedy` its `_argmax` twin (SPEC.md §24),
    which takes the same arguments without `head_io`'s actions_in, seed, offset and row_base."""
    fn = f"{name}_argmax" if greedy else name
    check(getattr(lib(), fn)(*args, *(io[4:] if greedy else io), _stream()), fn)


def _make_function():
    import torch

    class MaskedHeads(torch.autograd.Function):
        @staticmethod
        def forward(ctx, logits, mask, dims, action, seed, offset, row_base, greedy=False):
            hd = heads_struct(dims)
            total = sum(hd.dims[:hd.n_heads])
            if not logits.is_cuda or not mask.is_cuda:
                raise HeadsError("masked_heads runs on the GPU: logits and mask must be device tensors")
            if logits.dtype != torch.float32 or logits.dim() != 2 or logits.shape[1] != total:
                raise ValueError(f"logits must be float32 [N, {total}], got {logits.dtype} {tuple(logits.shape)}")
            n = logits.shape[0]
            logits, lstride = rows_arg(logits.detach(), total)
            mask, mptr, mstride, kind = _mask_arg(mask, n, total)
            dev = logits.device
            a_in, (a_out, logprob, entropy, lse, hent), io = head_io(action, n, hd.n_heads, dev, seed, offset, row_base)
            with torch.cuda.device(dev):
                forward_call("nmh_forward", greedy,
                             (ctypes.byref(hd), n, logits.data_ptr(), lstride, mptr, mstride, kind), io)
            ctx.hd, ctx.kind = hd, kind
            ctx.set_materialize_grads(False)  # an unused logprob / entropy arrives as None -> NULL
            ctx.save_for_backward(logits, mask, a_out, lse, hent)
            ctx.mark_non_differentiable(a_out, lse, hent)
            return a_out, logprob, entropy, lse, hent

        @staticmethod
        def backward(ctx, _ga, g_logprob, g_entropy, _gl, _gh):
            logits, mask, actions, lse, hent = ctx.saved_tensors
            hd = ctx.hd
            n, total = logits.shape
            g_logits = torch.empty((n, total), dtype=torch.float32, device=logits.device)
            glp = None if g_logprob is None else g_logprob.to(torch.float32).contiguous()
            gen = None if g_entropy is None else g_entropy.to(torch.float32).contiguous()
            with torch.cuda.device(logits.device):
                check(lib().nmh_backward(
                    ctypes.byref(hd), n, logits.data_ptr(), max(logits.stride(0), total), mask.data_ptr(),
                    max(mask.stride(0), total), ctx.kind, actions.data_ptr(), lse.data_ptr(), hent.data_ptr(),
                    ptr(glp), ptr(gen), g_logits.data_ptr(), total, _stream()), "nmh_backward")
            return g_logits, None, None, None, None, None, None, None

    return MaskedHeads


_function = None


def masked_heads_full(logits, mask, dims, action=None, *, seed: int = 0, offset: int = 0, row_base: int = 0,
                      greedy: bool = False):
    """`masked_heads` plus the per-head saved values: (action, logprob, entropy, lse [N, H],
    head_entropy [N, H])."""
    global _function
    check_greedy(greedy, action)
    if _function is None:
        _function = _make_function()
    a, logprob, entropy, lse, hent = _function.apply(logits, mask, tuple(dims), action, seed, offset, row_base,
                                                     bool(greedy))
    return (a if action is None else action), logprob, entropy, lse, hent


def masked_heads(logits, mask, dims, action=None, *, seed: int = 0, offset: int = 0, row_base: int = 0,
                 greedy: bool = False):
    """All masked categorical heads of a batch of rows in one kernel (SPEC.md §15).

    logits: float32 [N, sum(dims)] on the GPU, the heads' logits concatenated.
    mask: the flat obs tensor [N, obs_elems] float32 itself (its first sum(dims) columns are the
        ActionTargets, legal iff > 0, read in place), or a uint8 / bool [N, >= sum(dims)] tensor.
    action: None samples (int32 [N, H]; row r, head k draws from the philox counter
        (row_base + r, k, offset) under `seed`: the caller advances `offset` per call); else the
        given [N, H] actions are evaluated and returned as they are.
    greedy: with action None, select instead of sampling (SPEC.md §24): per head the smallest legal
        index whose logit is the head's maximum, 0 if nothing is legal; seed, offset and row_base
        are not used. logprob and entropy are those of evaluating the returned actions, and
        differentiable in the same way. With an action it is a ValueError.
    Returns (action, logprob [N], entropy [N]); logprob and entropy are sums over heads and
    differentiable with respect to logits.
    """
    return masked_heads_full(logits, mask, dims, action, seed=seed, offset=offset, row_base=row_base,
                             greedy=greedy)[:3]


# ---------------------------------------------------------------- pointer heads (SPEC.md §18)
def pointer_struct(dims, head_set, set_rows, key_dim) -> NmhPointer:
    head_set, set_rows = [int(s) for s in head_set], [int(m) for m in set_rows]
    if len(head_set) != len(dims):
        raise ValueError(f"head_set has {len(head_set)} entries for {len(dims)} heads")
    if len(set_rows) > MAX_SETS:
        raise ValueError(f"at most {MAX_SETS} key sets, got {len(set_rows)}")
    if set_rows and (key_dim % 4 or not 4 <= key_dim <= MAX_KEY_DIM):
        raise ValueError(f"the key width must be a multiple of 4 in 4..{MAX_KEY_DIM}, got {key_dim}")
    for k, s in enumerate(head_set):
        if not -1 <= s < len(set_rows):
            raise ValueError(f"head_set[{k}] = {s} names none of the {len(set_rows)} key sets")
        if s >= 0 and int(dims[k]) != set_rows[s] + 1:
            raise ValueError(f"head {k} has {dims[k]} entries, key set {s} has {set_rows[s]} rows + the no-op")
    if set(range(len(set_rows))) - set(head_set):
        raise ValueError(f"no head uses key set(s) {sorted(set(range(len(set_rows))) - set(head_set))}")
    if sum(int(d) for d in dims) > MAX_DIM:
        raise ValueError(f"the heads' sizes sum to {sum(dims)}, more than {MAX_DIM}")
    pt = NmhPointer()
    pt.n_sets, pt.key_dim = len(set_rows), int(key_dim)
    for s, m in enumerate(set_rows):
        pt.set_rows[s] = m
    for k, s in enumerate(head_set):
        pt.head_set[k] = s
    return pt


def _dense16(t):
    """t, detached, as a contiguous 16-byte aligned tensor (copied only if it is not one)."""
    t = t.detach().contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _key_array(tensors):
    return (ctypes.c_void_p * max(1, len(tensors)))(*[ptr(t) for t in tensors])


def _make_pointer_function():
    import torch

    class PointerHeads(torch.autograd.Function):
        @staticmethod
        def forward(ctx, queries, dense, mask, dims, head_set, action, seed, offset, row_base, *keys):
            # the selection mode, a bool, is the last argument where one is given (after the key tensors)
            greedy = bool(keys) and isinstance(keys[-1], bool) and keys[-1]
            keys = [kt for kt in keys if not isinstance(kt, bool)]
            hd = heads_struct(dims)
            dims, head_set = [int(d) for d in dims], [int(s) for s in head_set]
            if len(head_set) != len(dims):
                raise ValueError(f"head_set has {len(head_set)} entries for {len(dims)} heads")
            total, n_ptr = sum(dims), sum(s >= 0 for s in head_set)
            n_dense = sum(d for d, s in zip(dims, head_set) if s < 0)
            if not mask.is_cuda:
                raise HeadsError("pointer_heads runs on the GPU: every input must be a device tensor")
            n, dev = mask.shape[0], mask.device
            for s, kt in enumerate(keys):
                if not kt.is_cuda or kt.dtype != torch.float32 or kt.dim() != 3 or kt.shape[0] != n:
                    raise ValueError(f"keys[{s}] must be float32 [{n}, m, D] on the GPU, got {kt.dtype} {tuple(kt.shape)}")
            key_dim = keys[0].shape[2] if keys else 0
            if any(kt.shape[2] != key_dim for kt in keys):
                raise ValueError(f"every key set must have the same width, got {[kt.shape[2] for kt in keys]}")
            if n_ptr:
                if queries is None or not queries.is_cuda or queries.dtype != torch.float32 or \
                        tuple(queries.shape) != (n, n_ptr, key_dim):
                    raise ValueError(f"queries must be float32 [{n}, {n_ptr}, {key_dim}] on the GPU, got "
                                     f"{None if queries is None else (queries.dtype, tuple(queries.shape))}")
                queries = _dense16(queries)
            else:
                queries = None
            if n_dense:
                if dense is None or not dense.is_cuda or dense.dtype != torch.float32 or \
                        tuple(dense.shape) != (n, n_dense):
                    raise ValueError(f"dense_logits must be float32 [{n}, {n_dense}] on the GPU, got "
                                     f"{None if dense is None else (dense.dtype, tuple(dense.shape))}")
                dense = dense.detach().contiguous()
            else:
                dense = None
            keys = [_dense16(kt) for kt in keys]
            pt = pointer_struct(dims, head_set, [kt.shape[1] for kt in keys], key_dim)
            mask, mptr, mstride, kind = _mask_arg(mask, n, total)
            a_in, (a_out, logprob, entropy, lse, hent), io = head_io(action, n, hd.n_heads, dev, seed, offset, row_base)
            with torch.cuda.device(dev):
                forward_call("nmh_pointer_forward", greedy,
                             (ctypes.byref(hd), ctypes.byref(pt), n, ptr(queries), _key_array(keys), ptr(dense),
                              n_dense, mptr, mstride, kind), io)
            ctx.hd, ctx.pt, ctx.kind, ctx.n_dense = hd, pt, kind, n_dense
            ctx.has = (queries is not None, dense is not None)
            ctx.set_materialize_grads(False)
            ctx.save_for_backward(mask, a_out, lse, hent, *[t for t in (queries, dense) if t is not None], *keys)
            ctx.mark_non_differentiable(a_out, lse, hent)
            return a_out, logprob, entropy, lse, hent

        @staticmethod
        def backward(ctx, _ga, g_logprob, g_entropy, _gl, _gh):
            mask, actions, lse, hent, *rest = ctx.saved_tensors
            queries = rest.pop(0) if ctx.has[0] else None
            dense = rest.pop(0) if ctx.has[1] else None
            keys = rest
            hd, pt, n, dev = ctx.hd, ctx.pt, mask.shape[0], mask.device
            total = sum(hd.dims[:hd.n_heads])
            need = ctx.needs_input_grad  # a gradient nobody asked for is a NULL pointer: not computed
            g_q = torch.empty_like(queries) if queries is not None and need[0] else None
            g_d = torch.empty_like(dense) if dense is not None and need[1] else None
            g_k = [torch.empty_like(kt) if need[9 + s] else None for s, kt in enumerate(keys)]
            glp = None if g_logprob is None else g_logprob.to(torch.float32).contiguous()
            gen = None if g_entropy is None else g_entropy.to(torch.float32).contiguous()
            with torch.cuda.device(dev):
                check(lib().nmh_pointer_backward(
                    ctypes.byref(hd), ctypes.byref(pt), n, ptr(queries), _key_array(keys), ptr(dense), ctx.n_dense,
                    mask.data_ptr(), max(mask.stride(0), total), ctx.kind, actions.data_ptr(), lse.data_ptr(),
                    hent.data_ptr(), ptr(glp), ptr(gen), ptr(g_d), ctx.n_dense, ptr(g_q), _key_array(g_k), _stream()),
                    "nmh_pointer_backward")
            return (g_q, g_d, None, None, None, None, None, None, None, *g_k,
                    *[None] * (len(ctx.needs_input_grad) - 9 - len(g_k)))  # the mode, where it was passed

    return PointerHeads


_pointer_function = None


def pointer_heads_full(queries, keys, head_set, dense_logits, mask, dims, action=None, *, seed: int = 0,
                       offset: int = 0, row_base: int = 0, greedy: bool = False):
    """`pointer_heads` plus the per-head saved values: (action, logprob, entropy, lse [N, H],
    head_entropy [N, H])."""
    global _pointer_function
    check_greedy(greedy, action)
    if _pointer_function is None:
        _pointer_function = _make_pointer_function()
    a, logprob, entropy, lse, hent = _pointer_function.apply(
        queries, dense_logits, mask, tuple(dims), tuple(head_set), action, seed, offset, row_base, *keys, bool(greedy))
    return (a if action is None else action), logprob, entropy, lse, hent


def pointer_heads(queries, keys, head_set, dense_logits, mask, dims, action=None, *, seed: int = 0, offset: int = 0,
                  row_base: int = 0, greedy: bool = False):
    """Masked categorical heads of which some are pointer heads, in one kernel (SPEC.md §18): the
    decoders of the reference's policies (baseline_policy.py:222-230) without the zero-padded copy
    of the embeddings, the batched mat-vec over every candidate and the logits tensor.

    dims, head_set: per head its size and -1 (dense: its logits are given) or the index s of the
        key set it points into; then dims[k] == keys[s].shape[1] + 1, the last entry being the
        no-op with logit 0.
    queries: float32 [N, P, D], one query per pointer head in head order (None if P == 0).
    keys: a sequence of float32 [N, m_s, D]. Head k's logit of candidate j < m_s is
        keys[s][r, j] . queries[r, p]; rows of illegal candidates are never read.
    dense_logits: float32 [N, sum of the dense heads' dims] in head order, or None.
    mask, action, seed, offset, row_base, greedy: as for `masked_heads`; mask columns cover all heads.
    Returns (action, logprob [N], entropy [N]); logprob and entropy are differentiable with respect
    to queries, every keys tensor and dense_logits, and a gradient that nothing requires is not
    computed. Non-contiguous or misaligned inputs are copied; there is no torch fallback.
    """
    return pointer_heads_full(queries, keys, head_set, dense_logits, mask, dims, action, seed=seed, offset=offset,
                              row_base=row_base, greedy=greedy)[:3]
