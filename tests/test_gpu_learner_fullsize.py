"""The learner-side kernels at the C4 row count and at offsets past 2^31 elements / 2^32 bytes.

The C4 workload hands the learner one flat buffer of 1,024 envs x 128 agents = 131,072 rows of 23,987
float32 (3,144,024,064 elements, 12.6 GB). The unit tests of the kernels that read those rows in place
(test_gpu_heads / _pointer_heads / _tile / _item / _player / _storage_shapes) stop at 37 rows and pin
the compact call to float64; this module pins the same calls to the compact call, bit for bit, where
the row index times the row stride no longer fits 32 bits:

A. few rows, huge stride: `as_strided((9, 23987), (S, 1))` views of the big buffer with S odd (rows at
   all four alignments modulo 16 B) and chosen by `straddle` so that one row's section of interest
   (mask prefix, the pointer heads' 104 mask columns, Tile, Entity, Inventory, Market) contains element
   offset 2^31 ("e31": row 6, rows 7 and 8 lie wholly past it) or byte offset 2^32 ("b32": row 3, rows
   7 and 8 past 2^31 elements). The view starts at the buffer's first element, so the offsets the
   kernels form from their base pointer are the buffer's. int16 / uint8 views ("i16", "u8") put the
   boundary into the last row's section in buffers just past 2^31 elements of their type: there only
   the column offset added to the row's crosses 2^31, the product r * stride itself stays below it, so
   these cases exercise the other template instantiations' loads across the boundary and do not guard
   the row-times-stride product (the float32 views do). The wrappers' argument helpers must hand the view's own
   pointer on, and a call may allocate its outputs and nothing else (`grows`: the allocator's 512-B
   rounding of each listed tensor is the whole slack, so a hidden `.contiguous()` of nine sections
   does not fit). tests/test_learner_fullsize_geometry.py checks the geometry on the CPU.
B. the real row count: row r of the buffer holds pattern row r % 37 (37 is prime, so every pattern row
   meets every wave of a 4-row workgroup and every neighbour); each per-row entry point runs once over
   all 131,072 rows through its C entry point, into outputs with a canary margin at both ends, and
   output row r must equal output row r % 37 of the 37-row call, compared on the GPU in chunks.
   Sampled actions depend on the global row index (the Philox counter) and are checked with
   test_gpu_heads.check_samples on the first 37 rows, around both boundary rows and on the last 37,
   for the masked heads and, from materialised logits, for the pointer heads.
   After every single launch the buffer still holds the tiling, bit for bit.

The 37 pattern rows are real flat rows (offsets from `layout.flat_layout(2048)`) filled by the unit
tests' generators: test_gpu_heads.Case masks (all-zero, all-legal, first / last entry only, an empty
Buy head, an illegal given action) with test_gpu_player.mask_pattern over the pointer heads of rows
6..20, test_tile_abi.sample_tiles, test_gpu_player.make_sets (Entity, AgentId: every own-row case, NaN
class and id, +-32,767 columns, an all-zero set), test_gpu_item.make_sets (Inventory, Market). Row 0
is zero from end to end: an agent that is not in the realm.

Index audit, read before the first full-size run (r, m, n: row / set index; every line is 64-bit):
  heads.hip   nmh_forward_kernel      r0 = (int64_t)blockIdx.x * kRowsPerBlock + w
  heads.hip   nmh_forward_kernel      logits + r * ls; mask index r * ms + off + i (r, ls, ms int64_t)
  heads.hip   tile_heads              actions_in[r * n_heads + k]; q = r * n_heads + k (int64_t r)
  heads.hip   tile_heads              philox(row_base + (uint32_t)r, ..): a 32-bit counter by definition
  heads.hip   nmh_backward_kernel     logits + r * ls; g_logits + r * gs; r * ms + off + i; r * hd.n_heads + k
  heads.hip   nmh_pointer_* kernels   mbase = r * ms + off; dense + r * ds; g_dense + r * gds;
                                      (r * pl.n_ptr + src) * D; keys + r * m * D; gk + r * n4;
                                      k4[(int64_t)j * nd4 + d4]; staged + (size_t)w * wave_bytes
  tile_enc    nmh_tile_forward_kernel row0 = (int64_t)blockIdx.x * kFwdRows; tile + n * tile_stride;
                                      idx_out[n * kRowIdx + e]; out + n * kRowOut (n int64_t)
  item_enc    nmh_item_features       m = (int64_t)blockIdx.x * kSets + sub; items + m * item_stride;
                                      features + m * (int64_t)R * kF; set[(int64_t)j * kC + c]; sums[m * kF + t]
  item_enc    nmh_item_logits(_bwd)   r = (int64_t)blockIdx.x * kRowsPerBlock + w; items + (r / share) * item_stride;
                                      out + r * os; g_out + r * gs; r * ms + mask_off[h]; pq[r * H * kQ + i];
                                      g_pq[(r * H + h) * kQ + f]; set + (int64_t)j * kC
  player_enc  nmh_player_features     m = blockIdx.x (int64_t); ents + m * ent_stride; ids at m * id_stride;
                                      features + m * (int64_t)R * kF; sums[m * kF + tid]; mine + m * kF
  player_enc  nmh_player_own          m = (int64_t)blockIdx.x * kRowsPerBlock + w; ents + m * ent_stride; m * id_stride
  player_enc  nmh_player_logits(_bwd) r = (int64_t)blockIdx.x * kRowsPerBlock + w; ents + r * ent_stride; r * ms;
                                      out + r * os; g_out + r * gs; pq[r * H * kQ + i]; g_pq[(r * H + h) * kQ + f]
  storage.hip gather_rows_kernel      src + (size_t)idx[k] * words; out + (size_t)k * words (k int, < 2^31 / 4 rows)
  storage.hip store_rows_kernel       src + (size_t)r * elems; out + (size_t)s * elems (r, s int row numbers)
  wrappers    _mask_arg / _tile_arg / _item_arg / _ent_arg / _id_arg pass `stride(0)` as a Python int into an
              int64_t parameter (ctypes c_int64); gather passes row_bytes as int64_t. Grids are
              (n + 3) / 4 or n workgroups as unsigned: 32,768 or 131,072, far below 2^31.
No defect was found by reading, so no kernel or wrapper changes with this module.
"""

import contextlib
import ctypes
import time
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nmmo_amd import layout
from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

# ---------------------------------------------------------------- geometry (no GPU)
ROWS, K = 131072, 37
LAY = layout.flat_layout(2048)
W = LAY["__total__"].offset  # 23,987
DIMS = list(layout.ACTION_DIMS)
TOTAL = sum(DIMS)  # 1,586 mask entries lead a row
BIG = ROWS * W
E31, B32 = 1 << 31, 1 << 32
ROW_E31, ROW_B32 = E31 // W, (B32 // 4) // W  # the rows of the whole buffer that hold the two boundaries


def section(name):
    """(first column, columns) of a section of a flat row; "mask" is the ActionTargets prefix and "ptr"
    the part of it the pointer-heads case reads: its first two heads."""
    if name == "mask":
        return 0, TOTAL
    if name == "ptr":
        return 0, sum(DIMS[:2])
    seg = LAY[name]
    return seg.offset, int(np.prod(seg.shape))


Geometry = namedtuple("Geometry", "stride n width row target inside need itemsize")


def straddle(off, length, target, row, n, width, itemsize):
    """Rows of `width` elements at element offsets r * stride, r < n, of a buffer whose first row starts
    at its first element: an odd stride such that row `row`'s columns [off, off + length) contain element
    offset `target` (at column off + inside, near the middle). `need` is the elements the view spans."""
    q = target - off - length // 2
    stride = q // row
    stride -= stride % 2 == 0
    inside = target - off - row * stride  # = length // 2 + (0 .. 2 row - 1)
    return Geometry(stride, n, width, row, target, inside, (n - 1) * stride + width, itemsize)


N_A = 9  # rows of a view: two whole workgroups of four and a partial one
F32_SECTIONS = ["mask", "ptr", "Tile", "Entity", "Inventory", "Market"]
GEO = {}
for _name in F32_SECTIONS:
    _off, _len = section(_name)
    GEO[_name, "e31"] = straddle(_off, _len, E31, 6, N_A, W, 4)       # element offset 2^31
    GEO[_name, "b32"] = straddle(_off, _len, B32 // 4, 3, N_A, W, 4)  # byte offset 2^32
    if _name not in ("mask", "ptr"):  # int16 rows of the same layout: element 2^31 is also byte 2^32
        GEO[_name, "i16"] = straddle(_off, _len, E31, N_A - 1, N_A, W, 2)
GEO["mask", "u8"] = straddle(0, TOTAL, E31, N_A - 1, N_A, TOTAL, 1)
GEO["ptr", "u8"] = straddle(0, sum(DIMS[:2]), E31, N_A - 1, N_A, TOTAL, 1)
I16_ELEMS = max(g.need for (_, kind), g in GEO.items() if kind == "i16")
U8_ELEMS = max(g.need for (_, kind), g in GEO.items() if kind == "u8")
# pattern rows of a view's nine rows: the straddling rows 3, 6 and 8 hold dense ones
SEL = [0, 1, 2, 9, 4, 5, 30, 18, 12]
# the row gather: below, on and above both boundaries of the whole buffer, its first and last row
GATHER_ROWS = [0, ROW_B32 - 1, ROW_B32, ROW_B32 + 1, ROW_E31 - 1, ROW_E31, ROW_E31 + 1, ROWS - 1]
STORE_CAPACITY = ROW_E31 + 6  # experience rows: slots up to three past the 2^31 row

# ---------------------------------------------------------------- the heads of a flat row
HEAD_OFF = {f"{a}.{b}": LAY[f"ActionTargets.{a}.{b}"].offset for (a, b), _ in layout.ACTION_HEADS}
PLAYER_MOFF = [HEAD_OFF["Attack.Target"], HEAD_OFF["Give.Target"], HEAD_OFF["GiveGold.Target"]]
INV_MOFF = [HEAD_OFF[f"{a}.InventoryItem"] for a in ("Destroy", "Give", "Sell", "Use")]
MARKET_MOFF = [HEAD_OFF["Buy.MarketItem"]]
PDIMS, PSETS, PKEY = DIMS[:2], [-1, 0], 4  # pointer heads: Attack.Style dense, Attack.Target over 100 keys of 4
E_OFF, E_LEN = section("Entity")
I_OFF, I_LEN = section("Inventory")
M_OFF, M_LEN = section("Market")
T_OFF, T_LEN = section("Tile")
ID_OFF = LAY["AgentId"].offset
SEED, OFFSET = 0x1234567887654321, (3 << 32) + 17
CANARY, MARGIN = 7.5, 64
DEV = "cuda"
F32, I32, U8 = torch.float32, torch.int32, torch.uint8


# ---------------------------------------------------------------- pattern rows
class Patterns:
    """K flat rows and the per-row inputs of every entry point, on the GPU. nan=False leaves out the
    NaN class and id, for the int16 copy of the rows."""

    def __init__(self, nan):
        from tests import test_gpu_heads as th
        from tests import test_gpu_item as ti
        from tests import test_gpu_player as tp
        from tests.test_tile_abi import sample_tiles

        rng = np.random.default_rng(2031 + nan)
        hc = th.Case("nmmo", DIMS, K, 1.0, 2031)
        self.name, self.n, self.dims, self.slices = "fullsize", K, DIMS, hc.slices
        legal, actions = hc.legal.copy(), hc.actions_np.copy()
        for r in range(6, 21):  # the encoder tests' patterns over the pointer heads
            for k, ((_, arg), n) in enumerate(layout.ACTION_HEADS):
                if arg in ("Target", "MarketItem", "InventoryItem"):
                    sl = self.slices[k]
                    legal[r, sl] = tp.mask_pattern((r + k) % 5, n - 1, rng)
                    idx = np.flatnonzero(legal[r, sl])
                    actions[r, k] = rng.choice(idx) if len(idx) else rng.integers(n)
        self.legal, self.logits_np = legal, hc.logits_np
        rows = rng.integers(-9, 9, (K, W)).astype(np.float32)  # CurrentTick and Task: any values
        rows[:, :TOTAL] = np.where(legal, rng.choice([1.0, 0.5, 3.0], legal.shape), rng.choice([0.0, -1.0], legal.shape))
        ents, ids = tp.make_sets(K, 100, rng, nan=nan)
        rows[:, E_OFF:E_OFF + E_LEN] = ents.reshape(K, -1)
        rows[:, ID_OFF] = ids
        rows[:, I_OFF:I_OFF + I_LEN] = ti.make_sets(K, 12, rng, nan=nan).reshape(K, -1)
        rows[:, M_OFF:M_OFF + M_LEN] = ti.make_sets(K, 1024, rng, nan=nan).reshape(K, -1)
        rows[:, T_OFF:T_OFF + T_LEN] = sample_tiles(K, rng).reshape(K, -1)
        rows[0] = 0
        assert not legal[0].any() and legal[1].all() and np.nanmax(np.abs(rows[:, E_OFF:I_OFF])) == 32767
        assert np.isnan(rows).any() == bool(nan)
        self.rows = torch.from_numpy(rows).to(DEV)
        if not nan:
            self.rows16 = torch.from_numpy(rows.astype(np.int16)).to(DEV)
            self.u8 = torch.from_numpy(legal.astype(np.uint8) * 3).to(DEV)

        def normal(*shape):
            return torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(DEV)

        self.shared = dict(table=normal(3, 256, 9, 32), bias=normal(32))
        self.per_row = dict(
            logits=hc.logits.clone(), actions32=torch.from_numpy(actions.astype(np.int32)).to(DEV),
            glp=normal(K), gen=normal(K), queries=normal(K, 1, PKEY), keys=normal(K, 100, PKEY), dense=normal(K, 3),
            pq_player=normal(K, 3, 40), pq_inv=normal(K, 4, 36), pq_market=normal(K, 1, 36),
            g_player=normal(K, 3 * 101), g_inv=normal(K, 4 * 13), g_market=normal(K, 1025))

    def inputs(self, sel=None, n=None):
        """The per-row inputs of pattern rows `sel`, or of n rows holding pattern r % K."""
        x = SimpleNamespace(**self.shared)
        for name, t in self.per_row.items():
            if sel is not None:
                v = t[sel]
            elif n == K:
                v = t
            else:
                v = t.repeat(-(-n // K), *([1] * (t.dim() - 1)))[:n].contiguous()
            setattr(x, name, v)
        x.pactions32 = x.actions32[:, :2].contiguous()
        return x


_patterns = {}


def patterns(nan=True):
    if nan not in _patterns:
        _patterns[nan] = Patterns(nan)
    return _patterns[nan]


# ---------------------------------------------------------------- fixtures
STATS = dict(free0=0, min_free=1 << 62, t0=0.0)


def note_memory():
    STATS["min_free"] = min(STATS["min_free"], torch.cuda.mem_get_info()[0])


@pytest.fixture(scope="module")
def big():
    """The C4 flat buffer [131072, 23987] float32, mapped the way the engine maps its own."""
    from nmmo_amd import devmem

    free, _ = torch.cuda.mem_get_info()
    largest_out = ROWS * 32 * 13 * 13 * 4  # the tile forward's, 2.8 GB; the same again for a comparison
    need = BIG * 4 + 2 * largest_out + I16_ELEMS * 2 + U8_ELEMS + STORE_CAPACITY * W * 4 + (2 << 30)
    if free < need:
        pytest.skip(f"needs {need / 2**30:.1f} GiB of free device memory, {free / 2**30:.1f} GiB are free")
    STATS.update(free0=free, t0=time.time())
    buf = devmem.empty((ROWS, W), torch.float32, torch.device("cuda", torch.cuda.current_device()))
    state = SimpleNamespace(tiled=False)
    yield buf, state
    torch.cuda.synchronize()
    del buf
    devmem.release_pending()
    torch.cuda.empty_cache()
    print(f"\nlearner fullsize: wall {time.time() - STATS['t0']:.1f} s, peak device memory in use "
          f"{(STATS['free0'] - STATS['min_free']) / 2**30:.2f} GiB")


@pytest.fixture(scope="module")
def small(big):
    """Buffers just past 2^31 elements of int16 and of uint8."""
    b = SimpleNamespace(i16=torch.empty(I16_ELEMS, dtype=torch.int16, device=DEV),
                        u8=torch.empty(U8_ELEMS, dtype=torch.uint8, device=DEV))
    yield b
    del b.i16, b.u8
    torch.cuda.empty_cache()


def view_of(buf, geo, rows):
    """The strided view of `geo` over `buf`, its rows written."""
    v = buf.as_strided((geo.n, geo.width), (geo.stride, 1), buf.storage_offset())
    assert v.data_ptr() == buf.data_ptr() and geo.need <= buf.numel() and v.element_size() == geo.itemsize
    v.copy_(rows)
    return v


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, (i, a.shape, b.shape)
        assert torch.equal(bits(a.contiguous()), bits(b.contiguous())), f"output {i} differs"


@contextlib.contextmanager
def grows(measure, what, *allocs):
    """The call inside may raise the allocator's peak by the listed (shape, dtype) tensors, each rounded
    up to the allocator's 512 bytes, and by nothing else."""
    if not measure:
        yield
        return
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    yield
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    allowed = sum(-(-int(np.prod(shape)) * torch.empty((), dtype=dt).element_size() // 512) * 512 for shape, dt in allocs)
    print(f"{what}: the allocator's peak grew by {grew} B, outputs allow {allowed} B")
    assert grew <= allowed, (what, grew, allowed)


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------- A: the wrappers on a view
def run_masked(rows, x, measure):
    from nmmo_amd import heads

    n, H = rows.shape[0], len(DIMS)
    assert heads._mask_arg(rows, n, TOTAL)[1] == rows.data_ptr()
    five = [((n, H), I32), ((n,), F32), ((n,), F32), ((n, H), F32), ((n, H), F32)]
    lg = x.logits.clone().requires_grad_(True)
    with grows(measure, "masked_heads forward", *five):
        _, lp, ent, lse, hent = heads.masked_heads_full(lg, rows, DIMS, x.actions32)
    with grows(measure, "masked_heads backward", ((n, TOTAL), F32)):
        (g,) = torch.autograd.grad([lp, ent], [lg], [x.glp, x.gen])
    with grows(measure, "masked_heads sampled", *five):
        s = heads.masked_heads_full(x.logits, rows, DIMS, seed=SEED, offset=OFFSET)
    return [lp.detach(), ent.detach(), lse, hent, g, *s]


def run_pointer(rows, x, measure):
    from nmmo_amd import heads

    n, H = rows.shape[0], len(PDIMS)
    assert heads._mask_arg(rows, n, sum(PDIMS))[1] == rows.data_ptr()
    five = [((n, H), I32), ((n,), F32), ((n,), F32), ((n, H), F32), ((n, H), F32)]
    q, kk, d = (t.clone().requires_grad_(True) for t in (x.queries, x.keys, x.dense))
    with grows(measure, "pointer_heads forward", *five):
        _, lp, ent, lse, hent = heads.pointer_heads_full(q, [kk], PSETS, d, rows, PDIMS, x.pactions32)
    with grows(measure, "pointer_heads backward", (q.shape, F32), (kk.shape, F32), (d.shape, F32)):
        g = torch.autograd.grad([lp, ent], [q, kk, d], [x.glp, x.gen])
    with grows(measure, "pointer_heads sampled", *five):
        s = heads.pointer_heads_full(x.queries, [x.keys], PSETS, x.dense, rows, PDIMS, seed=SEED, offset=OFFSET)
    return [lp.detach(), ent.detach(), lse, hent, *g, *s]


def run_tile(rows, x, measure):
    from nmmo_amd import heads, tile

    n = rows.shape[0]
    sec = rows[:, T_OFF:T_OFF + T_LEN]
    arg, stride, kind = tile._tile_arg(sec, None)
    assert arg.data_ptr() == sec.data_ptr() == rows.data_ptr() + T_OFF * rows.element_size() and stride == rows.stride(0)
    tab = x.table.clone().requires_grad_(True)
    with grows(measure, "tile_conv1 with grad", ((n, 32, 13, 13), F32), ((n, 225, 3), U8)):
        out = tile.tile_conv1(sec, tab, x.bias)
    with torch.no_grad(), grows(measure, "tile_conv1 without grad", ((n, 32, 13, 13), F32)):
        out2 = tile.tile_conv1(sec, x.table, x.bias)
    out3 = torch.empty_like(out2)
    idx = torch.empty((n, 225, 3), dtype=U8, device=DEV)
    heads.check(heads.lib().nmh_tile_forward(n, ptr(arg), stride, kind, ptr(x.table), ptr(x.bias), ptr(out3), ptr(idx),
                                             stream()), "nmh_tile_forward")
    torch.cuda.synchronize()
    return [out.detach(), out2, out3, idx]


def run_item(rows, mask_rows, x, which, measure):
    from nmmo_amd import item

    n = rows.shape[0]
    off, R, moff, pq, g_out = (I_OFF, 12, INV_MOFF, x.pq_inv, x.g_inv) if which == "Inventory" else \
        (M_OFF, 1024, MARKET_MOFF, x.pq_market, x.g_market)
    sec = rows[:, off:off + 16 * R]
    arg, stride, r_, _ = item._item_arg(sec, None)
    assert arg.data_ptr() == sec.data_ptr() == rows.data_ptr() + off * rows.element_size()
    assert (stride, r_) == (rows.stride(0), R)
    outs = []
    with grows(measure, f"item_sums {which}", ((n, 32), F32)):
        outs.append(item.item_sums(sec))
    if which == "Inventory":
        with grows(measure, "item_features Inventory", ((n, R, 32), F32)):
            outs.append(item.item_features(sec))
    pq = pq.clone().requires_grad_(True)
    with grows(measure, f"item_logits {which}", ((n, len(moff) * (R + 1)), F32)):
        out = item.item_logits(sec, pq, mask_rows, moff)
    with grows(measure, f"item_logits backward {which}", (pq.shape, F32)):
        (g,) = torch.autograd.grad(out, pq, g_out)
    return outs + [out.detach(), g]


def run_player(rows, mask_rows, x, measure):
    from nmmo_amd import player

    n = rows.shape[0]
    sec, ids = rows[:, E_OFF:E_OFF + E_LEN], rows[:, ID_OFF]
    arg, stride, r_, _ = player._ent_arg(sec, None)
    assert arg.data_ptr() == sec.data_ptr() == rows.data_ptr() + E_OFF * rows.element_size()
    assert (stride, r_) == (rows.stride(0), 100)
    assert player._id_arg(ids, n)[0].data_ptr() == rows.data_ptr() + ID_OFF * rows.element_size()
    with grows(measure, "player_features", ((n, 100, 35), F32)):
        feats = player.player_features(sec)
    with grows(measure, "player_sums", ((n, 35), F32)):
        sums = player.player_sums(sec)
    with grows(measure, "player_own", ((n, 35), F32), ((n,), I32)):
        mine, idx = player.player_own(sec, ids)
    pq = x.pq_player.clone().requires_grad_(True)
    with grows(measure, "player_logits", ((n, 3 * 101), F32)):
        out = player.player_logits(sec, pq, mask_rows, PLAYER_MOFF)
    with grows(measure, "player_logits backward", (pq.shape, F32)):
        (g,) = torch.autograd.grad(out, pq, x.g_player)
    return [feats, sums, mine, idx, out.detach(), g]


def a_views(kind, name, big, small):
    """(the strided rows, their mask rows, the compact copies of both, the inputs) of one A case."""
    buf, state = big
    P = patterns(kind in ("e31", "b32"))
    x = P.inputs(sel=SEL)
    if kind in ("e31", "b32"):
        state.tiled = False
        compact = P.rows[SEL]
        v = view_of(buf.view(-1), GEO[name, kind], compact)
        return v, v, compact, compact, x
    cm = P.u8[SEL]
    vm = view_of(small.u8, GEO[name if name == "ptr" else "mask", "u8"], cm)
    if name in ("mask", "ptr"):
        return vm, vm, cm, cm, x
    compact = P.rows16[SEL]
    return view_of(small.i16, GEO[name, "i16"], compact), vm, compact, cm, x


def a_compare(fn, v, vm, compact, cm, x):
    got, want = fn(v, vm, x, True), fn(compact, cm, x, False)
    note_memory()
    same(got, want)
    assert torch.equal(bits(v), bits(compact)) and torch.equal(bits(vm), bits(cm)), "the rows were written"


@pytest.mark.parametrize("kind", ["e31", "b32", "u8"])
def test_a_masked_heads_on_a_straddling_view(kind, big, small):
    a_compare(lambda r, m, x, meas: run_masked(m, x, meas), *a_views(kind, "mask", big, small))


@pytest.mark.parametrize("kind", ["e31", "b32", "u8"])
def test_a_pointer_heads_on_a_straddling_view(kind, big, small):
    a_compare(lambda r, m, x, meas: run_pointer(m, x, meas), *a_views(kind, "ptr", big, small))


@pytest.mark.parametrize("kind", ["e31", "b32", "i16"])
def test_a_tile_conv1_on_a_straddling_view(kind, big, small):
    a_compare(lambda r, m, x, meas: run_tile(r, x, meas), *a_views(kind, "Tile", big, small))


@pytest.mark.parametrize("kind", ["e31", "b32", "i16"])
@pytest.mark.parametrize("which", ["Inventory", "Market"])
def test_a_item_encoder_on_a_straddling_view(which, kind, big, small):
    a_compare(lambda r, m, x, meas: run_item(r, m, x, which, meas), *a_views(kind, which, big, small))


@pytest.mark.parametrize("kind", ["e31", "b32", "i16"])
def test_a_player_encoder_on_a_straddling_view(kind, big, small):
    a_compare(lambda r, m, x, meas: run_player(r, m, x, meas), *a_views(kind, "Entity", big, small))


def test_a_gather_rows_around_both_boundaries(big):
    from nmmo_amd.storage import DeviceExperience

    buf, state = big
    state.tiled = False
    P = patterns()
    want = P.rows[SEL[:len(GATHER_ROWS)]]
    for r, row in zip(GATHER_ROWS, want):
        buf[r].copy_(row)
    idx = torch.tensor(GATHER_ROWS, dtype=I32, device=DEV)
    x = DeviceExperience(1, 1, 1)
    with grows(True, "gather", ((len(GATHER_ROWS), W), F32)):
        out = x.gather(buf, idx)
    note_memory()
    same([out], [want])
    for r, row in zip(GATHER_ROWS, want):
        assert torch.equal(bits(buf[r]), bits(row))


def test_a_store_rows_into_slots_past_both_boundaries(big):
    """nmmo_exp_store's row copy into experience slots around the rows of the storage that hold byte
    offset 2^32 and element offset 2^31: the write pointer is device memory the object owns."""
    from nmmo_amd import devmem
    from nmmo_amd.storage import DeviceExperience

    P = patterns()
    n = 7
    src = P.rows[SEL[2:2 + n]].contiguous()
    x = DeviceExperience(STORE_CAPACITY - 1, W, n)
    zeros, ones = torch.zeros(n, device=DEV), torch.ones(n, dtype=U8, device=DEV)
    for first in (ROW_B32 - 3, ROW_E31 - 3):
        x.reset()
        x.ptr_dev.fill_(first)
        x.store(src, zeros, zeros.to(U8), ones, torch.zeros((n, 12), dtype=I32, device=DEV), zeros, zeros, 0)
        note_memory()
        assert x.ptr == first + n and x.status == 0
        assert torch.equal(bits(x.obs[first:first + n]), bits(src))
        assert not x.obs[first - 1].any() and (first + n == x.capacity or not x.obs[first + n].any())
    del x
    torch.cuda.synchronize()
    devmem.release_pending()


# ---------------------------------------------------------------- B: the real row count
class Guarded:
    """Outputs with a canary margin at both ends."""

    def __init__(self):
        self.bufs = []

    def new(self, shape, dtype=F32):
        numel = int(np.prod(shape))
        fill = CANARY if dtype == F32 else 0x5A
        buf = torch.full((numel + 2 * MARGIN,), fill, dtype=dtype, device=DEV)
        self.bufs.append((buf, fill))
        return buf[MARGIN:MARGIN + numel].view(shape)

    def check(self):
        torch.cuda.synchronize()
        note_memory()
        for buf, fill in self.bufs:
            assert bool((buf[:MARGIN] == fill).all()) and bool((buf[-MARGIN:] == fill).all()), "a store outside the output"


def launched(after, rc, name):
    """One raw launch: its status, then the caller's check of the obs buffer."""
    from nmmo_amd import heads

    heads.check(rc, name)
    after(name)


def raw_masked(rows, n, x, after):
    from nmmo_amd import heads

    L, g, H = heads.lib(), Guarded(), len(DIMS)
    hd = heads.heads_struct(DIMS)
    _, mptr, ms, kind = heads._mask_arg(rows, n, TOTAL)
    assert mptr == rows.data_ptr() and ms == rows.stride(0)

    def five():
        return [g.new((n, H), I32), g.new((n,)), g.new((n,)), g.new((n, H)), g.new((n, H))]

    a, lp, ent, lse, hent = five()
    launched(after, L.nmh_forward(ctypes.byref(hd), n, ptr(x.logits), TOTAL, mptr, ms, kind, ptr(x.actions32), 0, 0, 0,
                              ptr(a), ptr(lp), ptr(ent), ptr(lse), ptr(hent), stream()), "nmh_forward")
    gl = g.new((n, TOTAL))
    launched(after, L.nmh_backward(ctypes.byref(hd), n, ptr(x.logits), TOTAL, mptr, ms, kind, ptr(x.actions32), ptr(lse),
                               ptr(hent), ptr(x.glp), ptr(x.gen), ptr(gl), TOTAL, stream()), "nmh_backward")
    s = five()
    launched(after, L.nmh_forward(ctypes.byref(hd), n, ptr(x.logits), TOTAL, mptr, ms, kind, None, SEED, OFFSET, 0,
                              *[ptr(t) for t in s], stream()), "nmh_forward")
    g.check()
    return [a, lp, ent, lse, hent, gl], s[0]


def raw_pointer(rows, n, x, after):
    from nmmo_amd import heads

    L, g, H = heads.lib(), Guarded(), len(PDIMS)
    hd = heads.heads_struct(PDIMS)
    pt = heads.pointer_struct(PDIMS, PSETS, [100], PKEY)
    _, mptr, ms, kind = heads._mask_arg(rows, n, sum(PDIMS))
    assert mptr == rows.data_ptr() and ms == rows.stride(0)
    a, lp, ent, lse, hent = g.new((n, H), I32), g.new((n,)), g.new((n,)), g.new((n, H)), g.new((n, H))
    keys = heads._key_array([x.keys])
    launched(after, L.nmh_pointer_forward(ctypes.byref(hd), ctypes.byref(pt), n, ptr(x.queries), keys, ptr(x.dense), 3, mptr,
                                      ms, kind, ptr(x.pactions32), 0, 0, 0, ptr(a), ptr(lp), ptr(ent), ptr(lse),
                                      ptr(hent), stream()), "nmh_pointer_forward")
    gq, gk, gd = g.new(x.queries.shape), g.new(x.keys.shape), g.new(x.dense.shape)
    launched(after, L.nmh_pointer_backward(ctypes.byref(hd), ctypes.byref(pt), n, ptr(x.queries), keys, ptr(x.dense), 3, mptr,
                                       ms, kind, ptr(x.pactions32), ptr(lse), ptr(hent), ptr(x.glp), ptr(x.gen), ptr(gd),
                                       3, ptr(gq), heads._key_array([gk]), stream()), "nmh_pointer_backward")
    s = [g.new((n, H), I32), g.new((n,)), g.new((n,)), g.new((n, H)), g.new((n, H))]
    launched(after, L.nmh_pointer_forward(ctypes.byref(hd), ctypes.byref(pt), n, ptr(x.queries), keys, ptr(x.dense), 3, mptr,
                                          ms, kind, None, SEED, OFFSET, 0, *[ptr(t) for t in s], stream()),
             "nmh_pointer_forward")
    g.check()
    return [a, lp, ent, lse, hent, gq, gk, gd], s[0]


def raw_tile(rows, n, x, after):
    from nmmo_amd import heads, tile

    g = Guarded()
    arg, stride, kind = tile._tile_arg(rows[:, T_OFF:T_OFF + T_LEN], None)
    assert arg.data_ptr() == rows.data_ptr() + 4 * T_OFF and stride == rows.stride(0)
    out, idx = g.new((n, 32, 13, 13)), g.new((n, 225, 3), U8)
    launched(after, heads.lib().nmh_tile_forward(n, ptr(arg), stride, kind, ptr(x.table), ptr(x.bias), ptr(out), ptr(idx),
                                             stream()), "nmh_tile_forward")
    g.check()
    return [out, idx], None


def raw_item(rows, n, x, after, which):
    from nmmo_amd import heads, item

    L, g = heads.lib(), Guarded()
    off, R, moff, pq, g_out = (I_OFF, 12, INV_MOFF, x.pq_inv, x.g_inv) if which == "Inventory" else \
        (M_OFF, 1024, MARKET_MOFF, x.pq_market, x.g_market)
    arg, stride, r_, kind = item._item_arg(rows[:, off:off + 16 * R], None)
    assert arg.data_ptr() == rows.data_ptr() + 4 * off and (stride, r_) == (rows.stride(0), R)
    H, width = len(moff), len(moff) * (R + 1)
    ih = item.item_heads_struct(moff, [h * (R + 1) for h in range(H)])
    _, mptr, ms, mkind = heads._mask_arg(rows, n, max(moff) + R + 1)
    assert mptr == rows.data_ptr()
    sums = g.new((n, 32))
    feats = g.new((n, R, 32)) if which == "Inventory" else None  # (Market's features would be 17 GB)
    launched(after, L.nmh_item_features(n, ptr(arg), stride, kind, R, ptr(feats), ptr(sums), stream()), "nmh_item_features")
    out, gpq = g.new((n, width)), g.new((n, H, 36))
    launched(after, L.nmh_item_logits(ctypes.byref(ih), n, ptr(arg), stride, kind, R, 1, mptr, ms, mkind, ptr(pq), ptr(out),
                                  width, stream()), "nmh_item_logits")
    launched(after, L.nmh_item_logits_backward(ctypes.byref(ih), n, ptr(arg), stride, kind, R, 1, mptr, ms, mkind, ptr(g_out),
                                           width, ptr(gpq), stream()), "nmh_item_logits_backward")
    g.check()
    return [sums, out, gpq] + ([feats] if feats is not None else []), None


def raw_player(rows, n, x, after):
    from nmmo_amd import heads, player

    L, g, R, H = heads.lib(), Guarded(), 100, 3
    arg, stride, r_, kind = player._ent_arg(rows[:, E_OFF:E_OFF + E_LEN], None)
    assert arg.data_ptr() == rows.data_ptr() + 4 * E_OFF and (stride, r_) == (rows.stride(0), R)
    ids, id_stride, id_kind = player._id_arg(rows[:, ID_OFF], n)
    assert ids.data_ptr() == rows.data_ptr() + 4 * ID_OFF and id_stride == rows.stride(0)
    ph = player.player_heads_struct(PLAYER_MOFF, [h * (R + 1) for h in range(H)])
    _, mptr, ms, mkind = heads._mask_arg(rows, n, max(PLAYER_MOFF) + R + 1)
    assert mptr == rows.data_ptr()
    feats, sums, mine, idx = g.new((n, R, 35)), g.new((n, 35)), g.new((n, 35)), g.new((n,), I32)
    launched(after, L.nmh_player_features(n, ptr(arg), stride, kind, R, None, 1, 0, ptr(feats), ptr(sums), None, None,
                                      stream()), "nmh_player_features")  # the workgroup-per-set kernel
    launched(after, L.nmh_player_features(n, ptr(arg), stride, kind, R, ptr(ids), id_stride, id_kind, None, None, ptr(mine),
                                      ptr(idx), stream()), "nmh_player_features")  # the wave-per-set own-row kernel
    out, gpq = g.new((n, H * (R + 1))), g.new((n, H, 40))
    launched(after, L.nmh_player_logits(ctypes.byref(ph), n, ptr(arg), stride, kind, R, mptr, ms, mkind, ptr(x.pq_player),
                                    ptr(out), H * (R + 1), stream()), "nmh_player_logits")
    launched(after, L.nmh_player_logits_backward(ctypes.byref(ph), n, ptr(arg), stride, kind, R, mptr, ms, mkind,
                                             ptr(x.g_player), H * (R + 1), ptr(gpq), stream()),
                "nmh_player_logits_backward")
    g.check()
    return [feats, sums, mine, idx, out, gpq], None


CHUNK = 64  # periods of K rows per comparison


def tiling_holds(got, ref):
    """got[r] == ref[r % K] for every row, bit for bit, K * CHUNK rows at a time."""
    n = got.shape[0]
    a, b = bits(got.reshape(n, -1)), bits(ref.reshape(K, -1))
    full = n // K
    body = a[:full * K].view(full, K, -1)
    for p in range(0, full, CHUNK):
        part = body[p:p + CHUNK]
        if not torch.equal(part, b.unsqueeze(0).expand_as(part)):
            return False
    return torch.equal(a[full * K:], b[:n - full * K])


@pytest.fixture
def tiled(big):
    buf, state = big
    P = patterns()
    if not state.tiled:
        full = ROWS // K
        buf[:full * K].view(full, K, W).copy_(P.rows.unsqueeze(0).expand(full, K, W))
        buf[full * K:].copy_(P.rows[:ROWS - full * K])
        state.tiled = True
    return buf, P


def b_compare(fn, tiled):
    buf, P = tiled
    keep = P.rows.clone()

    def small_unchanged(name):
        assert torch.equal(bits(P.rows), bits(keep)), f"{name} changed the 37 rows"

    def big_unchanged(name):
        assert tiling_holds(buf, P.rows), f"{name} changed the obs buffer"

    ref, ref_sampled = fn(P.rows, K, P.inputs(n=K), small_unchanged)
    x = P.inputs(n=ROWS)
    got, sampled = fn(buf, ROWS, x, big_unchanged)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a.shape[0] == ROWS and b.shape[0] == K and a.shape[1:] == b.shape[1:]
        assert tiling_holds(a, b), f"output {i}: a row differs from its pattern row's"
    return sampled, ref_sampled


def samples_follow_the_global_row(sampled, ref_sampled, dims, legal, logits_np):
    """The draws of rows 0..36, around both boundary rows and of the last 37 rows invert the CDF of their
    pattern row's logits under the Philox counter of their own row index."""
    from tests.test_gpu_heads import check_samples, head_slices

    assert torch.equal(sampled[:K], ref_sampled)
    for start in (0, ROW_B32 - 18, ROW_E31 - 18, ROWS - K):
        pat = (start + np.arange(K)) % K
        c = SimpleNamespace(name=f"rows {start}..{start + K - 1}", n=K, dims=dims, slices=head_slices(dims),
                            legal=legal[pat], logits_np=logits_np[pat])
        check_samples(c, sampled[start:start + K], SEED, OFFSET, start)


def test_b_masked_heads_over_every_row(tiled):
    sampled, ref_sampled = b_compare(raw_masked, tiled)
    P = tiled[1]
    samples_follow_the_global_row(sampled, ref_sampled, DIMS, P.legal, P.logits_np)


def test_b_pointer_heads_over_every_row(tiled):
    sampled, ref_sampled = b_compare(raw_pointer, tiled)
    P = tiled[1]
    # the logits the kernel forms, materialised the reference's way: the dense head as given, then
    # key . query over the 100 candidates and the no-op's 0
    q, keys, dense = (P.per_row[k].double().cpu().numpy() for k in ("queries", "keys", "dense"))
    logits = np.concatenate([dense, np.einsum("rjd,rd->rj", keys, q[:, 0]), np.zeros((K, 1))], 1)
    samples_follow_the_global_row(sampled, ref_sampled, PDIMS, P.legal[:, :sum(PDIMS)], logits)


def test_b_tile_forward_over_every_row(tiled):
    b_compare(raw_tile, tiled)


@pytest.mark.parametrize("which", ["Inventory", "Market"])
def test_b_item_encoder_over_every_row(which, tiled):
    b_compare(lambda rows, n, x, after: raw_item(rows, n, x, after, which), tiled)


def test_b_player_encoder_over_every_row(tiled):
    b_compare(raw_player, tiled)
