"""The reference's tile encoder (baseline_policy.py:85-112) with its embedding, first convolution
and ReLU fused into one HIP kernel (nmh_tile_forward / nmh_tile_backward of libnmmo_heads.so,
include/nmmo_heads.h, SPEC.md §19).

The embedding and `tile_conv_1` are both linear and the embedding's input is an index, so the two
collapse into a table that depends on the weights alone,

    T[f][v][k][o] = sum_e W1[o][f*32 + e][ky][kx] * E[f*256 + v][e]        (`tile_table`, plain torch)
    relu(conv1(embed(tile)))[n][o][y][x] = max(0, b1[o] + sum_{ky,kx,f} T[f][idx[n][(y+ky)*15 + x+kx][f]][ky*3+kx][o])

and `tile_conv1` is that lookup, a `torch.autograd.Function` whose backward gives the gradients of
T and b1; torch differentiates `tile_table` down to the two weights. The [N, 96, 15, 15] embedding
tensor (86,400 B per row) is never made: backward keeps the 675 index bytes of a row.

    enc = TileEncoder(256, fused=True).cuda()
    h = enc(obs, offset=layout.flat_layout(task_dim)["Tile"].offset)      # flat obs rows, read in place

`TileEncoder(fused=True, fused_conv2=True)` goes one layer further (`tile_conv12`, nmh_tile2_forward /
nmh_tile2_backward, SPEC.md §22): `tile_conv_2` and its ReLU run in the same kernel on the LDS copy
of the first convolution's result, so the [N, 32, 13, 13] activation (21,632 B per row) is never
written and only the [N, 8, 11, 11] that `tile_fc` consumes leaves the kernel; backward recomputes
the activation from the index bytes.

There is no torch fallback for the fused paths: a host tensor, or a missing library, is a `HeadsError`.
"""

from __future__ import annotations

import torch
from torch import nn
from torch.nn import functional as F

from . import heads
from .heads import HeadsError

TILES, FEATURES, VALUES, TAPS, CHANNELS, EMBED = 225, 3, 256, 9, 32, 32
SIDE, OUT_SIDE = 15, 13
ROW = TILES * FEATURES  # 675 entries of a row's Tile section
CENTRE = 112
FWD_ROWS = 4  # rows per workgroup of the forward kernel (NMH_TILE_FWD_ROWS)
MAX_CHUNKS = 64
CHUNK_ROWS = 16
TILE_F32, TILE_I16 = 0, 1
CHANNELS2, OUT2_SIDE = 8, 11  # tile_conv_2: 32 -> 8 channels, 13 x 13 -> 11 x 11 (NMH_TILE2_CHANNELS, NMH_TILE2_OUT)
FWD2_ROWS = 4  # rows per workgroup of the fused forward kernel (NMH_TILE2_FWD_ROWS)
MAX_W2_PARTS = 1024  # NMH_TILE2_MAX_PARTS
W2_PART_ROWS = 4


def n_chunks_for(n_rows: int) -> int:
    """The number of row chunks `tile_conv1`'s backward sums separately: ceil(N / 16), at most
    NMH_TILE_MAX_CHUNKS = 64. A function of N alone, so a given batch size always adds in the same
    order. 27 workgroups of 512 threads work on each chunk, two to a compute unit, so 16 rows per
    chunk put a workgroup on every one of 256 compute units from 152 rows on; at the cap the
    partial tables the caller adds are 64 x 884,736 B = 57 MB."""
    return max(1, min(MAX_CHUNKS, -(-int(n_rows) // CHUNK_ROWS)))


def n_w2_parts_for(n_rows: int) -> int:
    """The number of row parts `tile_conv12`'s backward sums `g_w2` and `g_bias2` over separately:
    ceil(N / 4), at most NMH_TILE2_MAX_PARTS = 1,024. A function of N alone, so a given batch size
    always adds in the same order. One workgroup of 256 threads works on a part, three to a compute
    unit by registers, so 1,024 parts are one full round over 256 compute units with one to spare
    and are reached at 4,096 rows, and a minibatch of 1,024 rows already gives every compute unit
    a workgroup. Four rows per part keep the part's own store (9,248 B) below a tenth of the
    4 x 21,632 B of `dz1` the same workgroup writes; at the cap the parts the caller adds are
    1,024 x 9,248 B = 9.5 MB, a sixth of the table's 57 MB."""
    return max(1, min(MAX_W2_PARTS, -(-int(n_rows) // W2_PART_ROWS)))


def tile_table(embedding_weight: torch.Tensor, conv1_weight: torch.Tensor) -> torch.Tensor:
    """T [3, 256, 9, 32] from the embedding's [768, 32] and tile_conv_1's [32, 96, 3, 3] weights;
    differentiable, any device and dtype."""
    E = embedding_weight.reshape(FEATURES, VALUES, EMBED)
    W = conv1_weight.reshape(CHANNELS, FEATURES, EMBED, TAPS)
    return torch.einsum("ofek,fve->fvko", W, E).contiguous()


def tile_indices(tile: torch.Tensor) -> torch.Tensor:
    """SPEC §19's index rule in torch, int64 [N, 225, 3], the reference's lines 96-98 without the
    in-place edit: for the unfused chain and for tests."""
    tile = tile.reshape(tile.shape[0], TILES, FEATURES)
    if tile.is_floating_point():
        rel = (tile[:, :, :2] - tile[:, CENTRE:CENTRE + 1, :2]) + 7
        t = torch.nan_to_num(torch.cat([rel, tile[:, :, 2:]], 2), nan=0.0).clip(0, 255).long()
    else:
        t = tile.to(torch.int32)
        t = torch.cat([t[:, :, :2] - t[:, CENTRE:CENTRE + 1, :2] + 7, t[:, :, 2:]], 2).clip(0, 255).long()
    return t


def _dense16(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().to(torch.float32).contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _tile_arg(x: torch.Tensor, kind):
    """(tensor kept alive, row stride in elements, NMH_TILE_*) of Tile sections read in place."""
    if x.dim() == 3 and tuple(x.shape[1:]) == (TILES, FEATURES) and x.stride(2) == 1 and x.stride(1) == FEATURES:
        x = x.as_strided((x.shape[0], ROW), (x.stride(0), 1), x.storage_offset())  # the same memory
    if x.dim() != 2 or x.shape[1] < ROW:
        raise ValueError(f"tile must be [N, >= {ROW}] or [N, {TILES}, {FEATURES}], got {tuple(x.shape)}")
    if x.dtype == torch.float32:
        want = TILE_F32
    elif x.dtype == torch.int16:
        want = TILE_I16
    else:
        raise TypeError(f"tile must be float32 or int16, got {x.dtype}")
    if kind is not None and kind != want:
        raise ValueError(f"kind {kind} does not match the tensor's dtype {x.dtype}")
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < ROW):
        x = x[:, :ROW].contiguous()
    return x, max(x.stride(0), ROW), want


class _TileConv1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, table, bias, kind):
        if not (x.is_cuda and table.is_cuda and bias.is_cuda):
            raise HeadsError("tile_conv1 runs on the GPU: tile, table and bias must be device tensors")
        if tuple(table.shape) != (FEATURES, VALUES, TAPS, CHANNELS) or tuple(bias.shape) != (CHANNELS,):
            raise ValueError(f"table must be [3, 256, 9, 32] and bias [32], got {tuple(table.shape)}, {tuple(bias.shape)}")
        x, stride, kind = _tile_arg(x.detach(), kind)
        n, dev = x.shape[0], x.device
        tab, b = _dense16(table), _dense16(bias)
        keep = any(ctx.needs_input_grad)  # all False under no_grad
        out = torch.empty((n, CHANNELS, OUT_SIDE, OUT_SIDE), dtype=torch.float32, device=dev)
        idx = torch.empty((n, TILES, FEATURES), dtype=torch.uint8, device=dev) if keep else None
        with torch.cuda.device(dev):
            heads.check(heads.lib().nmh_tile_forward(
                n, x.data_ptr(), stride, kind, tab.data_ptr(), b.data_ptr(), out.data_ptr(),
                None if idx is None else idx.data_ptr(), heads._stream()), "nmh_tile_forward")
        if keep:
            ctx.save_for_backward(idx, out)
        return out

    @staticmethod
    def backward(ctx, g_out):
        idx, out = ctx.saved_tensors
        n, dev = out.shape[0], out.device
        chunks = n_chunks_for(n)
        g_out = _dense16(g_out)
        g_table = torch.empty((chunks, FEATURES, VALUES, TAPS, CHANNELS), dtype=torch.float32, device=dev)
        g_bias = torch.empty((chunks, CHANNELS), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            heads.check(heads.lib().nmh_tile_backward(
                n, idx.data_ptr(), out.data_ptr(), g_out.data_ptr(), chunks, g_table.data_ptr(), g_bias.data_ptr(),
                heads._stream()), "nmh_tile_backward")
        if n == 0:
            g_table.zero_()
            g_bias.zero_()
        return None, g_table.sum(0), g_bias.sum(0), None


def tile_conv1(obs_or_tile: torch.Tensor, table: torch.Tensor, bias: torch.Tensor, *, kind=None) -> torch.Tensor:
    """relu(tile_conv_1(embedding(tile))) [N, 32, 13, 13] as one kernel (SPEC.md §19).

    obs_or_tile: the rows' Tile sections on the GPU, float32 (flat obs) or int16 (native obs), as
        [N, 225, 3] or as [N, >= 675] whose first 675 columns are the section. A view into the obs
        buffer (`obs[:, offset:offset + 675]`) is read in place, whatever its row stride and
        alignment, and never written.
    table: `tile_table(embedding.weight, tile_conv_1.weight)`; bias: `tile_conv_1.bias`.
    kind: None (from the dtype), TILE_F32 or TILE_I16.
    With grad enabled the kernel also stores the rows' indices (uint8 [N, 225, 3]); those and the
    output are all backward needs, so the obs buffer may be rewritten in between. The gradient is
    summed over `n_chunks_for(N)` chunks of rows without atomics: the same bits on every run."""
    return _TileConv1.apply(obs_or_tile, table, bias, kind)


class _TileConv12(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, table, bias1, weight2, bias2, kind):
        if not (x.is_cuda and table.is_cuda and bias1.is_cuda and weight2.is_cuda and bias2.is_cuda):
            raise HeadsError("tile_conv12 runs on the GPU: tile, table, weights and biases must be device tensors")
        if tuple(table.shape) != (FEATURES, VALUES, TAPS, CHANNELS) or tuple(bias1.shape) != (CHANNELS,):
            raise ValueError(f"table must be [3, 256, 9, 32] and bias1 [32], got {tuple(table.shape)}, {tuple(bias1.shape)}")
        if tuple(weight2.shape) != (CHANNELS2, CHANNELS, 3, 3) or tuple(bias2.shape) != (CHANNELS2,):
            raise ValueError(f"weight2 must be [8, 32, 3, 3] and bias2 [8], got {tuple(weight2.shape)}, {tuple(bias2.shape)}")
        x, stride, kind = _tile_arg(x.detach(), kind)
        n, dev = x.shape[0], x.device
        tab, b1, w2, b2 = _dense16(table), _dense16(bias1), _dense16(weight2), _dense16(bias2)
        keep = any(ctx.needs_input_grad)  # all False under no_grad
        out2 = torch.empty((n, CHANNELS2, OUT2_SIDE, OUT2_SIDE), dtype=torch.float32, device=dev)
        idx = torch.empty((n, TILES, FEATURES), dtype=torch.uint8, device=dev) if keep else None
        with torch.cuda.device(dev):
            heads.check(heads.lib().nmh_tile2_forward(
                n, x.data_ptr(), stride, kind, tab.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                out2.data_ptr(), None if idx is None else idx.data_ptr(), heads._stream()), "nmh_tile2_forward")
        if keep:
            ctx.save_for_backward(idx, out2, table, bias1, weight2)  # the last three are the caller's own tensors
        return out2

    @staticmethod
    def backward(ctx, g_out2):
        idx, out2, table, bias1, weight2 = ctx.saved_tensors
        tab, b1, w2 = _dense16(table), _dense16(bias1), _dense16(weight2)
        n, dev = out2.shape[0], out2.device
        chunks, parts = n_chunks_for(n), n_w2_parts_for(n)
        g_out2 = g_out2.detach().to(torch.float32).contiguous()

        def empty(*shape):
            return torch.empty(shape, dtype=torch.float32, device=dev)

        dz1 = empty(n, CHANNELS, OUT_SIDE, OUT_SIDE)  # transient: freed when backward returns
        g_table, g_bias1 = empty(chunks, FEATURES, VALUES, TAPS, CHANNELS), empty(chunks, CHANNELS)
        g_w2, g_bias2 = empty(parts, CHANNELS2, CHANNELS, 3, 3), empty(parts, CHANNELS2)
        with torch.cuda.device(dev):
            heads.check(heads.lib().nmh_tile2_backward(
                n, idx.data_ptr(), out2.data_ptr(), g_out2.data_ptr(), tab.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                chunks, parts, dz1.data_ptr(), g_table.data_ptr(), g_bias1.data_ptr(), g_w2.data_ptr(),
                g_bias2.data_ptr(), heads._stream()), "nmh_tile2_backward")
        if n == 0:
            for t in (g_table, g_bias1, g_w2, g_bias2):
                t.zero_()
        return None, g_table.sum(0), g_bias1.sum(0), g_w2.sum(0), g_bias2.sum(0), None


def tile_conv12(obs_or_tile: torch.Tensor, table: torch.Tensor, bias1: torch.Tensor, weight2: torch.Tensor,
                bias2: torch.Tensor, *, kind=None) -> torch.Tensor:
    """relu(tile_conv_2(relu(tile_conv_1(embedding(tile))))) [N, 8, 11, 11] as one kernel (SPEC.md §22).

    obs_or_tile, table, bias1 and kind as for `tile_conv1`; weight2 [8, 32, 3, 3] and bias2 [8] are
    `tile_conv_2`'s. The first convolution's [N, 32, 13, 13] result lives in LDS only. With grad
    enabled the call keeps the rows' indices (uint8 [N, 225, 3]), its output and references to
    `table`, `bias1` and `weight2`: backward recomputes the first activation from them, so the obs
    buffer may be rewritten in between. Backward allocates a transient [N, 32, 13, 13] buffer and sums
    the gradients over `n_chunks_for(N)` chunks (table, bias1) and `n_w2_parts_for(N)` parts
    (weight2, bias2) of rows without atomics: the same bits on every run."""
    return _TileConv12.apply(obs_or_tile, table, bias1, weight2, bias2, kind)


class TileEncoder(nn.Module):
    """The reference's TileEncoder (baseline_policy.py:85-112), parameter names and shapes included,
    so a `state_dict` moves both ways. `forward(obs, offset)` takes rows whose columns
    [offset, offset + 675) are the Tile section, the flat obs rows themselves or a [N, 225, 3] /
    [N, 675] tile tensor with offset 0, and does not write to them (the reference's forward edits
    its argument in place).

    `fused=False` is the reference's chain in torch. `fused=True` replaces embedding, `tile_conv_1`
    and the first ReLU by `tile_conv1`, reading the rows in place; `tile_conv_2` and `tile_fc` stay
    with torch. `fused_conv2=True` (needs `fused=True`) makes `forward` run `tile_conv_2` and its
    ReLU in the same kernel too (`tile_conv12`); `tile_fc` stays with torch."""

    def __init__(self, input_size: int, fused: bool = False, fused_conv2: bool = False):
        super().__init__()
        if fused_conv2 and not fused:
            raise ValueError("fused_conv2=True extends the fused path: it needs fused=True")
        self.fused = bool(fused)
        self.fused_conv2 = bool(fused_conv2)
        self.register_buffer("tile_offset", torch.tensor([i * VALUES for i in range(FEATURES)]), persistent=False)
        self.embedding = nn.Embedding(FEATURES * VALUES, EMBED)
        self.tile_conv_1 = nn.Conv2d(FEATURES * EMBED, CHANNELS, 3)
        self.tile_conv_2 = nn.Conv2d(CHANNELS, 8, 3)
        self.tile_fc = nn.Linear(8 * 11 * 11, input_size)

    def conv1(self, obs: torch.Tensor, offset: int = 0) -> torch.Tensor:
        """relu(tile_conv_1(embedding(tile))) [N, 32, 13, 13]: the part the kernel replaces."""
        if obs.dim() == 3:  # [N, 225, 3]: a view when contiguous
            obs = obs.reshape(obs.shape[0], -1)
        x = obs[:, offset:offset + ROW]  # a view: no [N, 225, 3] copy
        if self.fused:
            table = tile_table(self.embedding.weight, self.tile_conv_1.weight)
            return tile_conv1(x, table, self.tile_conv_1.bias)
        idx = tile_indices(x)
        tile = self.embedding(idx + self.tile_offset)
        agents, tiles, features, embed = tile.shape
        tile = tile.view(agents, tiles, features * embed).transpose(1, 2).view(agents, features * embed, SIDE, SIDE)
        return F.relu(self.tile_conv_1(tile))

    def forward(self, obs: torch.Tensor, offset: int = 0) -> torch.Tensor:
        if self.fused_conv2:
            if obs.dim() == 3:
                obs = obs.reshape(obs.shape[0], -1)
            table = tile_table(self.embedding.weight, self.tile_conv_1.weight)
            tile = tile_conv12(obs[:, offset:offset + ROW], table, self.tile_conv_1.bias, self.tile_conv_2.weight,
                               self.tile_conv_2.bias)
            return F.relu(self.tile_fc(tile.view(tile.shape[0], -1)))
        tile = F.relu(self.tile_conv_2(self.conv1(obs, offset)))
        tile = tile.contiguous().view(tile.shape[0], -1)
        return F.relu(self.tile_fc(tile))
