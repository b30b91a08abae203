"""Fused PPO minibatch loss: loader for libnmmo_ppo.so and `ppo_loss`, the
`torch.autograd.Function` over nmp_loss (include/nmmo_ppo.h, SPEC.md §16).

    loss, stats = ppo_loss(newlogprob, entropy, newvalue, old_logprob, advantages, returns,
                           old_values, clip_coef=0.1, vf_clip_coef=0.1, ent_coef=0.01, vf_coef=0.5)
    loss.backward()

replaces the chain of elementwise ops and reductions between the agent's forward and
`loss.backward()` (clean_pufferl.py:476-523, `DeviceTrainer.train`) by one kernel launch that
also leaves the gradients with respect to newlogprob, entropy and newvalue; backward only scales
them. There is no torch fallback: a missing or stale library is an error.

torch is imported first so that the library binds to the HIP runtime torch loaded (see
`_loader.py`): tensors' device pointers and torch's streams are then valid inside the library.
"""

from __future__ import annotations

import ctypes
import os

from . import _loader, build

LIB_PATH = os.environ.get("NMMO_PPO_LIB", build.lib_path("ppo"))
SYMBOLS = ["nmp_loss", "nmp_last_error", "nmp_build_info"]
NMP_OK, NMP_E_INVALID, NMP_E_HIP = 0, -1, -2
MAX_N = 1 << 24
# indices into `stats` (float32 [N_OUT]); the first N_STATS are what an accumulator sums
LOSS, PG_LOSS, V_LOSS, ENTROPY, OLD_APPROX_KL, APPROX_KL, CLIPFRAC, ADV_MEAN, ADV_STD = range(9)
N_STATS, N_OUT = 7, 9
_lib = None


class PpoError(RuntimeError):
    pass


class NmpParams(ctypes.Structure):
    _fields_ = [("clip_coef", ctypes.c_double), ("vf_clip_coef", ctypes.c_double), ("ent_coef", ctypes.c_double),
                ("vf_coef", ctypes.c_double), ("norm_adv", ctypes.c_int32), ("clip_vloss", ctypes.c_int32)]


def declare(L):
    L.nmp_loss.argtypes = [ctypes.POINTER(NmpParams), ctypes.c_int32] + [ctypes.c_void_p] * 14


def lib():
    global _lib
    if _lib is None:
        _lib = _loader.load("ppo", LIB_PATH, PpoError, "nmp", declare,
                            "there is no torch fallback for the fused loss")
    return _lib


def check(rc: int, what: str):
    if rc != NMP_OK:
        raise PpoError(f"{what} failed ({rc}): {lib().nmp_last_error().decode()}")


def params_struct(clip_coef, vf_clip_coef, ent_coef, vf_coef, norm_adv=True, clip_vloss=True) -> NmpParams:
    return NmpParams(float(clip_coef), float(vf_clip_coef), float(ent_coef), float(vf_coef), int(bool(norm_adv)),
                     int(bool(clip_vloss)))


def new_accumulator(device):
    """A zeroed float64 [N_STATS + 1] device accumulator for `ppo_loss(..., accum=)`: the sums of
    the calls' first N_STATS stats and, last, the number of calls."""
    import torch

    return torch.zeros(N_STATS + 1, dtype=torch.float64, device=device)


def _make_function():
    import torch

    class PpoLoss(torch.autograd.Function):
        @staticmethod
        def forward(ctx, newlogprob, entropy, newvalue, old_logprob, advantages, returns, old_values, params, accum):
            vecs = (newlogprob, entropy, newvalue, old_logprob, advantages, returns, old_values)
            names = ("newlogprob", "entropy", "newvalue", "old_logprob", "advantages", "returns", "old_values")
            n = newlogprob.shape[0] if newlogprob.dim() == 1 else -1
            for name, t in zip(names, vecs):
                if not t.is_cuda:
                    raise PpoError(f"ppo_loss runs on the GPU: {name} must be a device tensor")
                if t.dtype != torch.float32 or t.dim() != 1 or t.shape[0] != n:
                    raise ValueError(f"{name} must be float32 [N] like newlogprob, got {t.dtype} {tuple(t.shape)}")
            if n == 0:
                raise ValueError("ppo_loss of an empty minibatch is undefined")
            dev = newlogprob.device
            if accum is not None and (not accum.is_cuda or accum.dtype != torch.float64 or not accum.is_contiguous()
                                      or tuple(accum.shape) != (N_STATS + 1,)):
                raise ValueError(f"accum must be a contiguous float64 [{N_STATS + 1}] device tensor")
            vecs = [t.detach().contiguous() for t in vecs]
            loss = torch.empty((), dtype=torch.float32, device=dev)
            stats = torch.empty(N_OUT, dtype=torch.float32, device=dev)
            g = torch.empty((3, n), dtype=torch.float32, device=dev)  # every entry is stored by the kernel
            with torch.cuda.device(dev):
                check(lib().nmp_loss(
                    ctypes.byref(params), n, *[t.data_ptr() for t in vecs], loss.data_ptr(), stats.data_ptr(),
                    *[g[k].data_ptr() for k in range(3)], None if accum is None else accum.data_ptr(),
                    torch.cuda.current_stream().cuda_stream), "nmp_loss")
            ctx.save_for_backward(g)
            ctx.mark_non_differentiable(stats)
            return loss, stats

        @staticmethod
        def backward(ctx, g_loss, _g_stats):
            (g,) = ctx.saved_tensors
            scaled = g * g_loss  # one launch for the three vectors
            return scaled[0], scaled[1], scaled[2], None, None, None, None, None, None

    return PpoLoss


_function = None


def ppo_loss(newlogprob, entropy, newvalue, old_logprob, advantages, returns, old_values, *, clip_coef: float,
             vf_clip_coef: float, ent_coef: float, vf_coef: float, norm_adv: bool = True, clip_vloss: bool = True,
             accum=None):
    """The PPO minibatch loss, its statistics and its gradients in one kernel (SPEC.md §16).

    The seven vectors are float32 [N] on the GPU (non-contiguous ones are copied); the loss is
    differentiable with respect to newlogprob, entropy and newvalue, the other four are constants.
    accum: optional `new_accumulator(device)`; the call adds its first N_STATS stats and 1 to it
        on the device, so a loop of calls on one stream reads its means once at the end.
    Returns (loss, stats): a float32 scalar and the float32 [N_OUT] device tensor indexed by LOSS,
    PG_LOSS, V_LOSS, ENTROPY, OLD_APPROX_KL, APPROX_KL, CLIPFRAC, ADV_MEAN, ADV_STD.
    """
    global _function
    if _function is None:
        _function = _make_function()
    params = params_struct(clip_coef, vf_clip_coef, ent_coef, vf_coef, norm_adv, clip_vloss)
    return _function.apply(newlogprob, entropy, newvalue, old_logprob, advantages, returns, old_values, params, accum)
