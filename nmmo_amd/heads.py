"""Fused masked action heads: loader for libnmmo_heads.so and `masked_heads`, the
`torch.autograd.Function` over nmh_forward / nmh_backward (include/nmmo_heads.h, SPEC.md §15).

    action, logprob, entropy = masked_heads(logits, obs, dims)            # sample
    _, logprob, entropy = masked_heads(logits, obs, dims, action=action)  # evaluate, differentiable

replaces the per-head `masked_fill(mask == 0, -1e9)` + `Categorical` loop of the reference's
policies (baseline_policy.py:245-262) by one kernel forward and one backward. There is no torch
fallback: a missing or stale library is an error.

torch is imported first so that the library binds to the HIP runtime torch loaded (see
`_loader.py`): tensors' device pointers and torch's streams are then valid inside the library.
"""

from __future__ import annotations

import ctypes
import os

from . import _loader, build

LIB_PATH = os.environ.get("NMMO_HEADS_LIB", build.lib_path("heads"))
SYMBOLS = ["nmh_forward", "nmh_backward", "nmh_last_error", "nmh_build_info"]
MAX_HEADS, MAX_DIM = 16, 2048
MASK_F32, MASK_U8 = 0, 1
NMH_OK, NMH_E_INVALID, NMH_E_HIP = 0, -1, -2
_lib = None


class HeadsError(RuntimeError):
    pass


class NmhHeads(ctypes.Structure):
    _fields_ = [("n_heads", ctypes.c_int32), ("dims", ctypes.c_int32 * MAX_HEADS)]


def declare(L):
    vp, i32, i64, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
    hp = ctypes.POINTER(NmhHeads)
    L.nmh_forward.argtypes = [hp, i32, vp, i64, vp, i64, i32, vp, u64, u64, ctypes.c_uint32, vp, vp, vp, vp, vp, vp]
    L.nmh_backward.argtypes = [hp, i32, vp, i64, vp, i64, i32, vp, vp, vp, vp, vp, vp, i64, vp]


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
    if mask.stride(1) != 1 or (n_rows > 1 and mask.stride(0) < total):
        mask = mask[:, :total].contiguous()
    return mask, mask.data_ptr(), max(mask.stride(0), total), kind


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _make_function():
    import torch

    class MaskedHeads(torch.autograd.Function):
        @staticmethod
        def forward(ctx, logits, mask, dims, action, seed, offset, row_base):
            hd = heads_struct(dims)
            total = sum(hd.dims[:hd.n_heads])
            if not logits.is_cuda or not mask.is_cuda:
                raise HeadsError("masked_heads runs on the GPU: logits and mask must be device tensors")
            if logits.dtype != torch.float32 or logits.dim() != 2 or logits.shape[1] != total:
                raise ValueError(f"logits must be float32 [N, {total}], got {logits.dtype} {tuple(logits.shape)}")
            n = logits.shape[0]
            logits = logits.detach()
            if logits.stride(1) != 1 or (n > 1 and logits.stride(0) < total):
                logits = logits.contiguous()
            mask, mptr, mstride, kind = _mask_arg(mask, n, total)
            dev = logits.device
            a_in = None
            if action is not None:
                if tuple(action.shape) != (n, hd.n_heads):
                    raise ValueError(f"action must be [{n}, {hd.n_heads}], got {tuple(action.shape)}")
                a_in = action.to(device=dev, dtype=torch.int32).contiguous()
            a_out = torch.empty((n, hd.n_heads), dtype=torch.int32, device=dev)
            logprob = torch.empty(n, dtype=torch.float32, device=dev)
            entropy = torch.empty(n, dtype=torch.float32, device=dev)
            lse = torch.empty((n, hd.n_heads), dtype=torch.float32, device=dev)
            hent = torch.empty((n, hd.n_heads), dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                check(lib().nmh_forward(
                    ctypes.byref(hd), n, logits.data_ptr(), max(logits.stride(0), total), mptr, mstride, kind,
                    None if a_in is None else a_in.data_ptr(), int(seed) & (2**64 - 1), int(offset) & (2**64 - 1),
                    int(row_base) & 0xFFFFFFFF, a_out.data_ptr(), logprob.data_ptr(), entropy.data_ptr(),
                    lse.data_ptr(), hent.data_ptr(), _stream()), "nmh_forward")
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
                    None if glp is None else glp.data_ptr(), None if gen is None else gen.data_ptr(),
                    g_logits.data_ptr(), total, _stream()), "nmh_backward")
            return g_logits, None, None, None, None, None, None

    return MaskedHeads


_function = None


def masked_heads_full(logits, mask, dims, action=None, *, seed: int = 0, offset: int = 0, row_base: int = 0):
    """`masked_heads` plus the per-head saved values: (action, logprob, entropy, lse [N, H],
    head_entropy [N, H])."""
    global _function
    if _function is None:
        _function = _make_function()
    a, logprob, entropy, lse, hent = _function.apply(logits, mask, tuple(dims), action, seed, offset, row_base)
    return (a if action is None else action), logprob, entropy, lse, hent


def masked_heads(logits, mask, dims, action=None, *, seed: int = 0, offset: int = 0, row_base: int = 0):
    """All masked categorical heads of a batch of rows in one kernel (SPEC.md §15).

    logits: float32 [N, sum(dims)] on the GPU, the heads' logits concatenated.
    mask: the flat obs tensor [N, obs_elems] float32 itself (its first sum(dims) columns are the
        ActionTargets, legal iff > 0, read in place), or a uint8 / bool [N, >= sum(dims)] tensor.
    action: None samples (int32 [N, H]; row r, head k draws from the philox counter
        (row_base + r, k, offset) under `seed`: the caller advances `offset` per call); else the
        given [N, H] actions are evaluated and returned as they are.
    Returns (action, logprob [N], entropy [N]); logprob and entropy are sums over heads and
    differentiable with respect to logits.
    """
    return masked_heads_full(logits, mask, dims, action, seed=seed, offset=offset, row_base=row_base)[:3]
