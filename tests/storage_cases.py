"""Case table for the experience-storage kernels (nmmo_amd/csrc/storage.hip): store, the
(env_id, step) sort, GAE and the row gathers, at the shapes where their block and chunk structure
can go wrong. numpy / torch-CPU only. tests/test_storage_cases.py checks on the CPU that every
case has the property its name claims; tests/test_gpu_storage_shapes.py replays the cases into
DeviceExperience and oracle/storage.py ReferenceStorage and compares bit for bit.

  S  store cases: a list of recvs and a batch_size. The count/place passes work in blocks of
     BLOCK = 512 rows; the cases put the capacity cut in a named block, leave blocks without a
     selected row, and (the large case) give a thread more than one block total to add up.
  K  sort cases: the S cases; sort_scan walks n_slots in chunks of 512 with a carry.
  G  GAE cases: (B, rewards, values, dones, idxs, gamma, gae_lambda); the kernel walks chunks of
     64 with a partial last chunk.
  R  gather cases: row widths around the 8 x 64-dword unrolled body and its 64-stride tail, row
     counts around the 4 rows of a block.
"""

from __future__ import annotations

from collections import namedtuple

import numpy as np

BLOCK = 512  # rows per workgroup in store_count / store_place, slots per chunk in sort_scan
HEADS = 12

Recv = namedtuple("Recv", "mask rewards dones actions logprobs values env_id base step obs")
# cut: the claim about where the capacity cut of recv number cut_recv falls (checked on the CPU):
#   None (no selected row is cut), ("block", k), "boundary" or "above512".
# oob: rows of the last recv whose env_id lies outside [0, n_slots).
# second: the recvs of a second batch, stored after sort() and reset() on the same object.
StoreCase = namedtuple("StoreCase", "name batch_size E n_slots recvs cut cut_recv oob second chunks3")
GaeCase = namedtuple("GaeCase", "name B rewards values dones idxs gamma gae_lambda kind")
GatherCase = namedtuple("GatherCase", "name src idx words")

GAE_PAIRS = [(0.99, 0.95), (1.0, 1.0), (0.0, 0.5), (0.9, 0.8), (0.995, 0.97)]
GAE_SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 1000, 4097]
WIDTHS = [1, 2, 63, 64, 65, 447, 448, 449, 511, 512, 513, 1023, 1025]  # dwords per row
COUNTS = [1, 3, 4, 5, 9]


def ids_of(rv: Recv) -> np.ndarray:
    n = len(rv.mask)
    return rv.env_id if rv.env_id is not None else rv.base + np.arange(n, dtype=np.int32)


def selected_per_block(mask) -> np.ndarray:
    m = np.asarray(mask, dtype=np.int64)
    pad = (-len(m)) % BLOCK
    return np.concatenate([m, np.zeros(pad, dtype=np.int64)]).reshape(-1, BLOCK).sum(1)


# ------------------------------------------------------------------------------------ store (S, K)
def _recv(rng, mask, E, step, n_slots, ids="base", base=0, tag=0):
    """One recv of len(mask) rows. ids: "base" (env_id_base + row), "perm" (an explicit random
    choice of distinct ids that holds 0 and n_slots - 1) or an explicit array. obs elements are
    distinct integers (exact in float32), different for every recv of a case through `tag`."""
    mask = np.asarray(mask, dtype=np.uint8)
    n = len(mask)
    env_id = None
    if isinstance(ids, np.ndarray):
        env_id = ids.astype(np.int32)
    elif ids == "perm":
        assert n <= n_slots
        env_id = rng.permutation(n_slots)[:n].astype(np.int32)
        if n >= 2:  # ids 0 and n_slots - 1 on selected rows where there are any
            sel = np.flatnonzero(mask)
            a, b = (sel[0], sel[-1]) if len(sel) >= 2 else (0, n - 1)
            for row, want in ((a, 0), (b, n_slots - 1)):
                at = np.flatnonzero(env_id == want)
                if len(at):
                    env_id[at[0]] = env_id[row]
                env_id[row] = want
    else:
        assert base >= 0 and base + n <= n_slots
    obs = (np.arange(n * E, dtype=np.int64) + tag * 20011 + 7).astype(np.float32).reshape(n, E)
    assert obs.max() < 2 ** 24
    return Recv(mask=mask,
                rewards=rng.standard_normal(n).astype(np.float32),
                dones=(rng.random(n) < 0.3).astype(np.uint8),
                actions=rng.integers(0, 120, (n, HEADS)).astype(np.int32),
                logprobs=rng.standard_normal(n).astype(np.float32),
                values=rng.standard_normal(n).astype(np.float32),
                env_id=env_id, base=base, step=step, obs=obs)


def _rand_mask(rng, n, p=0.7):
    return (rng.random(n) < p).astype(np.uint8)


def _n_sel(recvs):
    return int(sum(int(r.mask.sum()) for r in recvs))


def _case(name, recvs, n_slots, E, batch_size=None, cut=None, cut_recv=None, oob=(), second=None):
    if batch_size is None:  # room for every selected row of either batch
        batch_size = max(_n_sel(recvs), _n_sel(second or []), 1) + 2
    return StoreCase(name, int(batch_size), E, n_slots, recvs, cut, cut_recv, tuple(oob), second,
                     n_slots > 2 * BLOCK)


def _cut_case(name, seed, room_of, cut, ids="base", E=3):
    """A 513-row recv that leaves ptr0 > 0, then a 1537-row recv (four blocks: 512, 512, 512, 1)
    whose capacity cut is set through room_of(per-block selected counts) = the room left."""
    rng = np.random.default_rng(seed)
    n_slots = 1537
    a = _recv(rng, _rand_mask(rng, 513), E, 1, n_slots, ids="perm", tag=0)
    m = _rand_mask(rng, 1537)
    m[0] = m[1023] = m[1024] = m[1536] = 1
    b = _recv(rng, m, E, 2, n_slots, ids=ids, tag=1)
    room = int(room_of(selected_per_block(m)))
    capacity = int(a.mask.sum()) + room
    return _case(name, [a, b], n_slots, E, batch_size=capacity - 1, cut=cut, cut_recv=1)


def store_cases():
    out = []
    # all-ones masks at every row count, n_slots at the chunk edges, several rows per id
    for i, (n, n_slots, ids) in enumerate([(511, 511, "base"), (512, 512, "perm"), (513, 513, "base"),
                                           (1024, 1024, "perm"), (1537, 1537, "base")]):
        rng = np.random.default_rng(100 + i)
        recvs = [_recv(rng, np.ones(n, np.uint8), 2, s + 1, n_slots, ids=ids, tag=s) for s in range(3)]
        second = [_recv(rng, _rand_mask(rng, n), 2, s + 1, n_slots, ids=ids, tag=3 + s) for s in range(2)]
        out.append(_case(f"ones_{n}_slots{n_slots}", recvs, n_slots, 2, second=second))
    # random ~0.7 masks, explicit permuted ids
    for i, (n, n_slots) in enumerate([(511, 1025), (513, 1537), (1024, 1025), (1537, 1537)]):
        rng = np.random.default_rng(200 + i)
        recvs = [_recv(rng, _rand_mask(rng, n), 3, s + 1, n_slots, ids="perm", tag=s) for s in range(3)]
        out.append(_case(f"random_{n}_slots{n_slots}", recvs, n_slots, 3))
    # sparse ids: 511 of 1537 ids, each selected with p = 0.15, in four steps; then a second batch
    rng = np.random.default_rng(300)
    ids = np.sort(rng.permutation(1537)[:511]).astype(np.int32)
    ids[0], ids[-1] = 0, 1536
    mk = lambda: np.concatenate([[1], _rand_mask(rng, 509, 0.15), [1]])  # noqa: E731
    recvs = [_recv(rng, mk(), 1, s + 1, 1537, ids=ids, tag=s) for s in range(4)]
    second = [_recv(rng, mk(), 1, s + 1, 1537, ids=ids[::-1].copy(), tag=4 + s) for s in range(3)]
    out.append(_case("sparse_511_slots1537", recvs, 1537, 1, second=second))
    # blocks without a selected row: an all-zero recv between two stores, only the last row (blocks
    # 0..2 empty), a whole middle block masked off
    rng = np.random.default_rng(400)
    last = np.zeros(1537, np.uint8)
    last[-1] = 1
    mid = _rand_mask(rng, 1537)
    mid[512:1024] = 0
    mid[511] = mid[1024] = 1
    recvs = [_recv(rng, _rand_mask(rng, 513), 3, 1, 1537, ids="perm", tag=0),
             _recv(rng, np.zeros(1024, np.uint8), 3, 2, 1537, ids="base", tag=1),
             _recv(rng, last, 3, 3, 1537, ids="base", tag=2),
             _recv(rng, mid, 3, 4, 1537, ids="perm", tag=3)]
    out.append(_case("empty_blocks_1537", recvs, 1537, 3))
    # the capacity cut of a four-block store that starts at ptr0 > 0
    out.append(_cut_case("cut_in_block0", 500, lambda c: c[0] // 2, ("block", 0)))
    out.append(_cut_case("cut_on_block_boundary", 501, lambda c: c[0] + c[1], "boundary", ids="perm"))
    out.append(_cut_case("cut_in_block2", 502, lambda c: c[0] + c[1] + c[2] // 2, ("block", 2)))
    out.append(_cut_case("cut_in_last_block", 503, lambda c: c[0] + c[1] + c[2], ("block", 3), ids="perm"))
    out.append(_cut_case("cut_room1", 504, lambda c: 1, ("block", 0)))
    out.append(_cut_case("cut_room0", 505, lambda c: 0, ("block", 0), ids="perm"))
    # two selected rows of blocks 1 and 2 with an env_id outside [0, n_slots)
    rng = np.random.default_rng(600)
    m = _rand_mask(rng, 1537)
    m[700] = m[1300] = 1
    a = _recv(rng, _rand_mask(rng, 513), 3, 1, 1537, ids="base", tag=0)
    b = _recv(rng, m, 3, 2, 1537, ids="perm", tag=1)
    b.env_id[700], b.env_id[1300] = 1537, -7
    out.append(_case("env_id_out_of_range", [a, b], 1537, 3, oob=(700, 1300)))
    out.append(_large_case())
    return out


def _large_case():
    """512 * 512 + 513 rows = 514 blocks: the threads of block 513 add up two block totals each
    (blocks tid and tid + 512). The cut falls in block 513 (the last row, selected, has no room)."""
    rng = np.random.default_rng(700)
    n = BLOCK * BLOCK + 513
    a = _recv(rng, np.ones(511, np.uint8), 1, 1, n, ids="base", tag=0)
    m = _rand_mask(rng, n, 0.5)
    m[-1] = 1
    b = _recv(rng, m, 1, 2, n, ids="base", tag=1)
    capacity = 511 + int(m.sum()) - 1
    return _case("large_cut_above_block_512", [a, b], n, 1, batch_size=capacity - 1, cut="above512", cut_recv=1)


def reference_mask(case: StoreCase, rv: Recv) -> np.ndarray:
    """The mask the reference is fed: the rows with an out-of-range env_id cleared (the device
    drops them and raises status bit 0; the reference knows no such rows)."""
    m = rv.mask.copy()
    if case.oob and rv is case.recvs[-1]:
        m[list(case.oob)] = 0
    return m


def row_width_cases():
    """store_rows_kernel at the gather widths: 5 rows with 3 selected, twice (ptr0 = 0 and 3)."""
    out = []
    for w in WIDTHS:
        rng = np.random.default_rng(800 + w)
        recvs = [_recv(rng, [1, 0, 1, 1, 0], w, 1, 5, tag=0), _recv(rng, [0, 1, 1, 0, 1], w, 2, 5, tag=1)]
        out.append(_case(f"row_width_{w}", recvs, 5, w))
    return out


# ------------------------------------------------------------------------------------------ GAE (G)
def _gae(name, seed, B, pair, dones, kind):
    rng = np.random.default_rng(seed)
    n = B + 1
    if kind == "normal":
        rewards, values = rng.standard_normal(n), rng.standard_normal(n)
    elif kind == "large":  # no overflow beyond +-inf and no inf - inf: checked on the CPU
        rewards, values = rng.standard_normal(n), 1e30 * rng.standard_normal(n)
    elif kind == "subnormal":
        rewards = 1e-41 * rng.choice([-1.0, 1.0, 2.0], n)
        values = 3e-42 * rng.choice([-1.0, 1.0, 3.0], n)
    else:  # "zeros": exact zeros of both signs
        rewards = np.where(rng.random(n) < 0.5, 0.0, -0.0)
        values = np.where(rng.random(n) < 0.5, 0.0, -0.0)
    d = {"none": np.zeros(n), "all": np.ones(n), "half": (rng.random(n) < 0.5)}[dones]
    return GaeCase(name, B, rewards.astype(np.float32), values.astype(np.float32), d.astype(np.float32),
                   rng.permutation(n).astype(np.int32), pair[0], pair[1], kind)


def gae_cases():
    """Every size, constant pair, dones pattern and value kind occurs; the cross product is not
    taken (the reference loop costs ~70 us per row): sizes cycle through the pairs and dones
    patterns, and at B = 129 (two full chunks and one element) and 65 every pair meets every
    value kind and every dones pattern."""
    out = []
    modes = ["half", "none", "all"]
    for i, B in enumerate(GAE_SIZES):
        pair = GAE_PAIRS[(i + 3) % 5]  # 1000 gets (1.0, 1.0) and 4097 (0.0, 0.5); a second pair each below
        out.append(_gae(f"B{B}_g{pair[0]}_l{pair[1]}_{modes[i % 3]}", 1000 + i, B, pair, modes[i % 3], "normal"))
    out.append(_gae("B4097_g0.9_l0.8_half", 1100, 4097, (0.9, 0.8), "half", "normal"))
    out.append(_gae("B1000_g0.995_l0.97_half", 1101, 1000, (0.995, 0.97), "half", "normal"))
    for p, pair in enumerate(GAE_PAIRS):
        for k, kind in enumerate(["large", "subnormal", "zeros"]):
            for m, mode in enumerate(modes):
                B = 129 if (k + m) % 2 == 0 else 65
                out.append(_gae(f"B{B}_g{pair[0]}_l{pair[1]}_{mode}_{kind}", 1200 + 9 * p + 3 * k + m, B, pair,
                                mode, kind))
    return out


# --------------------------------------------------------------------------------------- gather (R)
def _index_vector(count, n_src, style):
    if style == "reversed":  # descending from the last source row, wrapping (repeats when count > n_src)
        return ((n_src - 1 - np.arange(count)) % n_src).astype(np.int32)
    rng = np.random.default_rng(count * 31 + n_src)
    idx = rng.integers(0, n_src, count)
    idx[-1] = n_src - 1
    if count >= 3:
        idx[0] = idx[1]  # a repeat
    return idx.astype(np.int32)


def gather_cases():
    """src as numpy arrays [n_src, cols] of float32 / int32 / int64 / uint8 with rows of `words`
    dwords; int64 rows exist only at even widths (row_bytes is a multiple of 8 there)."""
    out = []
    n_src = 7
    for wi, w in enumerate(WIDTHS):
        for ci, count in enumerate(COUNTS):
            style = "reversed" if (wi + ci) % 2 else "random"
            idx = _index_vector(count, n_src, style)
            src = (np.arange(n_src * w, dtype=np.int64).reshape(n_src, w) * 3 + 1).astype(np.float32) * 0.5
            out.append(GatherCase(f"float32_w{w}_n{count}", src, idx, w))
        count = COUNTS[wi % 5]
        idx = _index_vector(count, n_src, "random")
        rng = np.random.default_rng(900 + w)
        out.append(GatherCase(f"int32_w{w}_n{count}", rng.integers(-2 ** 31, 2 ** 31, (n_src, w)).astype(np.int32),
                              idx, w))
        out.append(GatherCase(f"uint8_w{w}_n{count}", rng.integers(0, 256, (n_src, 4 * w)).astype(np.uint8),
                              _index_vector(count, n_src, "reversed"), w))
        if w % 2 == 0:
            out.append(GatherCase(f"int64_w{w}_n{count}",
                                  rng.integers(-2 ** 62, 2 ** 62, (n_src, w // 2)).astype(np.int64), idx, w))
    return out


# -------------------------------------------------------------------------- the reference's results
def reference_store(ref, case: StoreCase, rv: Recv) -> int:
    """One recv into a ReferenceStorage; returns the rows kept."""
    return ref.store(rv.obs, rv.rewards, rv.dones, reference_mask(case, rv), rv.actions, rv.logprobs, rv.values,
                     ids_of(rv), rv.step)


_GAE_REF = {}


def gae_reference(c: GaeCase):
    """The reference's advantages of a G case (float32 torch CPU tensor [B]), computed once."""
    if c.name not in _GAE_REF:
        import torch

        from oracle.storage import ReferenceStorage

        ref = ReferenceStorage(c.B, 1)
        ref.rewards[:] = torch.from_numpy(c.rewards)
        ref.values[:] = torch.from_numpy(c.values)
        ref.dones[:] = torch.from_numpy(c.dones)
        _GAE_REF[c.name] = ref.advantages(c.idxs.tolist(), c.gamma, c.gae_lambda)
    return _GAE_REF[c.name]
