"""Fused LSTM recurrence: loader for libnmmo_lstm.so and `LSTM`, a drop-in for a time-first
`torch.nn.LSTM` over nml_cell / nml_seq_forward / nml_seq_backward (include/nmmo_lstm.h,
SPEC.md §17).

    rnn = LSTM(256, 256).cuda()
    rnn.load_state_dict(torch_lstm.state_dict())          # torch.nn.LSTM's names and shapes
    y, (h, c) = rnn(x, (h0, c0))                           # x [T, B, I], state [num_layers, B, H]
    with torch.no_grad():
        y, state = rnn(x, state, out=state)                # the state table updated in place

With grad enabled a layer is one `torch.autograd.Function`: one GEMM for `x W_ih^T` over the
window, one launch for the T steps, and in backward one launch plus the GEMMs that reduce over
rows. Under `torch.no_grad()` a step is `addmm_` plus the elementwise cell kernel. Grad mode
decides, not a size. There is no torch fallback: a missing or stale library is an error, and so is
a host tensor.

torch is imported first so that the library binds to the HIP runtime torch loaded (see
`_loader.py`): tensors' device pointers and torch's streams are then valid inside the library.
"""

from __future__ import annotations

import ctypes
import math
import os

import torch
from torch import nn

from . import _loader, build

LIB_PATH = os.environ.get("NMMO_LSTM_LIB", build.lib_path("lstm"))
SYMBOLS = ["nml_cell", "nml_seq_forward", "nml_seq_backward", "nml_last_error", "nml_build_info"]
NML_OK, NML_E_INVALID, NML_E_HIP = 0, -1, -2
H_STEP, MAX_H, MAX_B, MAX_T = 64, 1024, 1 << 24, 4096
ROWS = 4  # batch rows per workgroup of the sequence kernels
_lib = None


class LstmError(RuntimeError):
    pass


def declare(L):
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.nml_cell.argtypes = [i32, i32] + [vp] * 9
    L.nml_seq_forward.argtypes = [i32, i32, i32] + [vp] * 12
    L.nml_seq_backward.argtypes = [i32, i32, i32] + [vp] * 11


def lib():
    global _lib
    if _lib is None:
        _lib = _loader.load("lstm", LIB_PATH, LstmError, "nml", declare,
                            "there is no torch fallback for the fused LSTM")
    return _lib


def check(rc: int, what: str):
    if rc != NML_OK:
        raise LstmError(f"{what} failed ({rc}): {lib().nml_last_error().decode()}")


def _dev(name: str, t: torch.Tensor, shape) -> torch.Tensor:
    """`t` as a contiguous float32 device tensor of `shape` (a copy only if it is not contiguous)."""
    if not t.is_cuda:
        raise LstmError(f"the fused LSTM runs on the GPU: {name} must be a device tensor")
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be float32 {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def cell(ga, gb, b_ih, b_hh, c_prev, h_out, c_out, gates_out=None):
    """nml_cell on the current stream: `ga` [B, 4H] (+ `gb`, `b_ih`, `b_hh`, each or None) and
    `c_prev` [B, H] into `h_out`, `c_out` (which may be `c_prev`) and, if given, `gates_out`. The
    tensors must be contiguous float32 device tensors; nothing is copied or allocated."""
    B, H = c_prev.shape
    for name, t, shape in (("ga", ga, (B, 4 * H)), ("gb", gb, (B, 4 * H)), ("b_ih", b_ih, (4 * H,)),
                           ("b_hh", b_hh, (4 * H,)), ("c_prev", c_prev, (B, H)), ("h_out", h_out, (B, H)),
                           ("c_out", c_out, (B, H)), ("gates_out", gates_out, (B, 4 * H))):
        if t is not None and _dev(name, t, shape) is not t:
            raise ValueError(f"{name} must be contiguous")
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    with torch.cuda.device(c_prev.device):
        check(lib().nml_cell(B, H, ptr(ga), ptr(gb), ptr(b_ih), ptr(b_hh), ptr(c_prev), ptr(h_out), ptr(c_out),
                             ptr(gates_out), _stream()), "nml_cell")


class _LayerFunction(torch.autograd.Function):
    """One layer over a window: (x [T, B, I], W_ih, W_hh, b_ih, b_hh, h0, c0) -> (y, h_T, c_T)."""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, h0, c0):
        T, B, I = x.shape
        H = w_hh.shape[1]
        x, w_ih, w_hh = _dev("x", x, (T, B, I)), _dev("weight_ih", w_ih, (4 * H, I)), _dev("weight_hh", w_hh, (4 * H, H))
        b_ih, b_hh = _dev("bias_ih", b_ih, (4 * H,)), _dev("bias_hh", b_hh, (4 * H,))
        h0, c0 = _dev("h0", h0, (B, H)), _dev("c0", c0, (B, H))
        xg = (x.view(T * B, I) @ w_ih.t()).view(T, B, 4 * H)
        whh_t = w_hh.t().contiguous()  # [H, 4H]: the layout nml_seq_forward reads coalesced
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)  # noqa: E731
        y, gates, cs = new(T, B, H), new(T, B, 4 * H), new(T, B, H)  # every entry is stored by the kernel
        h_T, c_T = new(B, H), new(B, H)
        with torch.cuda.device(x.device):
            check(lib().nml_seq_forward(T, B, H, *[t.data_ptr() for t in (xg, whh_t, b_ih, b_hh, h0, c0, y, h_T, c_T,
                                                                          gates, cs)], _stream()), "nml_seq_forward")
        ctx.save_for_backward(x, w_ih, w_hh, h0, c0, y, gates, cs)
        return y, h_T, c_T

    @staticmethod
    def backward(ctx, dy, dh_T, dc_T):
        x, w_ih, w_hh, h0, c0, y, gates, cs = ctx.saved_tensors
        T, B, I = x.shape
        H = w_hh.shape[1]
        dy, dh_T, dc_T = _dev("dy", dy, (T, B, H)), _dev("dh_T", dh_T, (B, H)), _dev("dc_T", dc_T, (B, H))
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)  # noqa: E731
        dG, dh0, dc0 = new(T, B, 4 * H), new(B, H), new(B, H)
        with torch.cuda.device(x.device):
            check(lib().nml_seq_backward(T, B, H, *[t.data_ptr() for t in (dy, dh_T, dc_T, gates, cs, c0, w_hh, dG,
                                                                           dh0, dc0)], _stream()), "nml_seq_backward")
        # The reductions over the T * B rows: one GEMM or sum each. The two weight GEMMs run in
        # float64: a float32 GEMM adds a column's T * B products in one chain, which at 1,040 rows
        # is 3 to 5 times the error of a blocked sum, and these matrices are small.
        dG2 = dG.view(T * B, 4 * H)
        h_prev = torch.cat([h0.unsqueeze(0), y[:-1]]).view(T * B, H)
        dGt = dG2.t().double()
        db = dG2.sum(0)
        return ((dG2 @ w_ih).view(T, B, I), (dGt @ x.view(T * B, I).double()).float(),
                (dGt @ h_prev.double()).float(), db, db.clone(), dh0, dc0)


class LSTM(nn.Module):
    """A time-first `torch.nn.LSTM(input_size, hidden_size, num_layers)` (with biases, one
    direction, no dropout, no projection) whose recurrence runs in libnmmo_lstm.so. Parameter
    names, shapes and initialisation are torch.nn.LSTM's, so a `state_dict` moves both ways."""

    def __init__(self, input_size: int, hidden_size: int, num_layers: int = 1):
        super().__init__()
        if hidden_size % H_STEP or not H_STEP <= hidden_size <= MAX_H:
            raise ValueError(f"hidden_size {hidden_size} is not a multiple of {H_STEP} in {H_STEP}..{MAX_H}")
        if num_layers < 1 or input_size < 1:
            raise ValueError("num_layers and input_size must be at least 1")
        self.input_size, self.hidden_size, self.num_layers = int(input_size), int(hidden_size), int(num_layers)
        for k in range(num_layers):
            n_in = input_size if k == 0 else hidden_size
            for name, shape in ((f"weight_ih_l{k}", (4 * hidden_size, n_in)),
                                (f"weight_hh_l{k}", (4 * hidden_size, hidden_size)),
                                (f"bias_ih_l{k}", (4 * hidden_size,)), (f"bias_hh_l{k}", (4 * hidden_size,))):
                setattr(self, name, nn.Parameter(torch.empty(shape)))
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.hidden_size)
        for p in self.parameters():
            nn.init.uniform_(p, -bound, bound)

    def layer_parameters(self, k: int):
        return [getattr(self, f"{n}_l{k}") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]

    def forward(self, x, state=None, out=None):
        """x [T, B, input_size]; state (h0, c0), each [num_layers, B, H], or None for zeros.
        Returns (y [T, B, H], (h_T, c_T)).

        out: under `torch.no_grad()` only, an (h, c) pair of contiguous [num_layers, B, H] tensors
            that receive the new state and are returned as it; it may be `state` itself, which is
            then updated in place. With T == 1, `y` is a view of the last layer's `out[0]` rather
            than a copy."""
        if x.dim() != 3 or x.shape[2] != self.input_size:
            raise ValueError(f"x must be [T, B, {self.input_size}], got {tuple(x.shape)}")
        T, B, _ = x.shape
        L, H = self.num_layers, self.hidden_size
        if not x.is_cuda:
            raise LstmError("the fused LSTM runs on the GPU: x must be a device tensor")
        if T < 1:
            raise ValueError("x holds no step")
        if state is None:
            zeros = torch.zeros((L, B, H), dtype=torch.float32, device=x.device)
            state = (zeros, zeros)
        h0, c0 = (_dev(n, t, (L, B, H)) for n, t in zip(("h0", "c0"), state))
        if torch.is_grad_enabled():
            if out is not None:
                raise ValueError("out= writes the state in place: use it under torch.no_grad()")
            hs, cs = [], []
            for k in range(L):
                x, h, c = _LayerFunction.apply(x, *self.layer_parameters(k), h0[k], c0[k])
                hs.append(h)
                cs.append(c)
            return x, (torch.stack(hs), torch.stack(cs))
        return self._steps(_dev("x", x, x.shape), h0, c0, out)

    def _steps(self, x, h0, c0, out):
        T, B, _ = x.shape
        L, H = self.num_layers, self.hidden_size
        if out is None:
            out = (torch.empty_like(h0), torch.empty_like(c0))
        h_out, c_out = out
        for name, t in (("out[0]", h_out), ("out[1]", c_out)):
            if _dev(name, t, (L, B, H)) is not t:
                raise ValueError(f"{name} must be contiguous")
        if c_out.data_ptr() != c0.data_ptr():
            c_out.copy_(c0)  # the steps then update c in place
        for k in range(L):
            w_ih, w_hh, b_ih, b_hh = self.layer_parameters(k)
            xg = (x.view(T * B, -1) @ w_ih.t()).view(T, B, 4 * H)
            # y[t] is h_t; the last step goes straight to out[0][k], which may be the h it read
            y = h_out[k].unsqueeze(0) if T == 1 else torch.empty((T, B, H), dtype=torch.float32, device=x.device)
            h = h0[k]
            for t in range(T):
                xg[t].addmm_(h, w_hh.t())  # ordered before the cell on the stream
                cell(xg[t], None, b_ih, b_hh, c_out[k], y[t], c_out[k])
                h = y[t]
            if T > 1:
                h_out[k].copy_(y[T - 1])
            x = y
        return x, (h_out, c_out)
