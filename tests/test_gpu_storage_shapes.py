"""The experience-storage kernels (nmmo_amd/csrc/storage.hip) at multi-block and chunk-edge
shapes: the cases of tests/storage_cases.py (checked on the CPU by tests/test_storage_cases.py)
replayed into DeviceExperience and into the reference's storage restated on the CPU
(oracle/storage.py). Store placement over several blocks of 512 rows with the capacity cut in a
named block, the sort's chunked scan, GAE at partial chunks and constant pairs that tell the
reference's rounding apart, row copies around the unrolled body's width, and store_many with two
blocks per input. Every comparison is bit-exact."""

import numpy as np
import pytest

from oracle.storage import ReferenceStorage
from tests import storage_cases as sc

pytestmark = pytest.mark.gpu

S = sc.store_cases()
W = sc.row_width_cases()
G = sc.gae_cases()
R = sc.gather_cases()
FIELDS = ("obs", "actions", "logprobs", "rewards", "dones", "truncateds", "values")


def _same(a, b, what):
    import torch

    a = a.cpu()
    b = torch.as_tensor(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    assert torch.equal(a, b), f"{what} differs at {(a != b).nonzero()[:5].tolist()}"


def _store(x, rv):
    import torch

    t = torch.from_numpy
    x.store(t(rv.obs).to(x.device), t(rv.rewards), t(rv.dones), t(rv.mask), t(rv.actions), t(rv.logprobs),
            t(rv.values), rv.step, env_id=None if rv.env_id is None else t(rv.env_id), env_id_base=rv.base)


def _replay_batch(x, ref, case, recvs):
    """Store recvs on both sides, compare every buffer and the sort keys, then sort both."""
    import torch

    for k, rv in enumerate(recvs):
        _store(x, rv)
        sc.reference_store(ref, case, rv)
        assert x.ptr == ref.ptr, f"{case.name}: ptr after recv {k}: {x.ptr} != {ref.ptr}"
    n = ref.ptr
    for name in FIELDS:
        _same(getattr(x, name), getattr(ref, name), f"{case.name}: {name}")
    ids = np.array([k[0] for k in ref.sort_keys], dtype=np.int64).reshape(-1)
    steps = np.array([k[1] for k in ref.sort_keys], dtype=np.int64).reshape(-1)
    seen, seq = {}, []
    for i in ids.tolist():  # the running count of each id
        seq.append(seen.get(i, 0))
        seen[i] = seq[-1] + 1
    _same(x.env_id[:n].long(), ids, f"{case.name}: env_id")
    _same(x.step[:n].long(), steps, f"{case.name}: step")
    _same(x.seq[:n].long(), np.array(seq, dtype=np.int64), f"{case.name}: seq")
    _same(x.slot_count.long(), np.bincount(ids, minlength=case.n_slots), f"{case.name}: slot_count")
    assert x.status == (1 if case.oob else 0), f"{case.name}: status {x.status}"
    order = x.sort()
    _same(order.long(), torch.tensor(ref.sort(), dtype=torch.int64), f"{case.name}: sorted idxs")
    assert not x.slot_count.any(), f"{case.name}: slot_count after sort"


def _replay(case):
    from nmmo_amd.storage import DeviceExperience

    x = DeviceExperience(case.batch_size, case.E, case.n_slots)
    ref = ReferenceStorage(case.batch_size, case.E)
    _replay_batch(x, ref, case, case.recvs)
    if case.second:  # a second batch after reset() on the same object
        x.reset()
        ref.ptr = 0  # :200; sort() emptied the keys (:415)
        assert not ref.sort_keys
        _replay_batch(x, ref, case, case.second)


@pytest.mark.parametrize("case", S, ids=[c.name for c in S])
def test_store_and_sort_match_reference(case):
    _replay(case)


@pytest.mark.parametrize("case", W, ids=[c.name for c in W])
def test_store_rows_at_row_widths(case):
    """store_rows_kernel's 8 x 64-dword body and 64-stride tail at the gather widths."""
    _replay(case)


@pytest.mark.parametrize("case", G, ids=[c.name for c in G])
def test_gae_matches_reference(case):
    import torch

    from nmmo_amd.storage import DeviceExperience

    x = DeviceExperience(case.B, 1, 1)
    x.rewards.copy_(torch.from_numpy(case.rewards))
    x.values.copy_(torch.from_numpy(case.values))
    x.dones.copy_(torch.from_numpy(case.dones))
    idxs = torch.from_numpy(case.idxs).to(x.device)
    adv = x.advantages(idxs, case.gamma, case.gae_lambda)
    _same(adv, sc.gae_reference(case), f"{case.name}: advantages")


def test_gather_matches_indexing():
    import torch

    from nmmo_amd.storage import DeviceExperience

    x = DeviceExperience(1, 1, 1)
    for c in R:
        src = torch.from_numpy(c.src)
        idx = torch.from_numpy(c.idx)
        out = x.gather(src.to(x.device), idx.to(x.device))
        assert out.dtype == src.dtype
        _same(out, src[idx.long()], c.name)


def test_gather_writes_only_its_rows():
    """nmmo_gather_rows on buffers with a guard row behind the source and the output: the n rows
    equal src[idx] and the guard row keeps its fill. A wave that copies a dword too many (the
    unrolled body taken at j + 7 * 64 == words) lands in the guard row, whatever the order in
    which the rows' waves finish."""
    import ctypes

    import torch

    from nmmo_amd._native import check, lib

    dev = torch.device("cuda", torch.cuda.current_device())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for c in R:
        rows = torch.from_numpy(c.src).view(len(c.src), -1).view(torch.uint8)  # [n_src, 4 * words]
        n, row_bytes = len(c.idx), 4 * c.words
        src = torch.cat([rows, torch.full((1, row_bytes), 0x5A, dtype=torch.uint8)]).to(dev)
        out = torch.full((n + 1, row_bytes), 0xA5, dtype=torch.uint8, device=dev)
        idx = torch.from_numpy(c.idx).to(dev)
        check(lib().nmmo_gather_rows(ctypes.c_void_p(src.data_ptr()), row_bytes, ctypes.c_void_p(idx.data_ptr()), n,
                                     ctypes.c_void_p(out.data_ptr()), stream), "nmmo_gather_rows")
        _same(out[:n], rows[torch.from_numpy(c.idx).long()], c.name)
        assert bool((out[n] == 0xA5).all()), f"{c.name}: a write behind the last row"


def test_store_many_two_blocks_per_input_matches_reference():
    """store_count_many / store_place_many with gridDim.x = 2: three wire engines of 5 envs (640
    rows = two blocks per input), the packed 8-B smalls, the capacity cut in the second block of
    input 1. Against ReferenceStorage fed the same masks, fields and env_id_base + row ids, its obs
    rows the wire buffer unpacked and expanded."""
    import torch

    from nmmo_amd import abi, wire
    from nmmo_amd.config import Config
    from nmmo_amd.engine import NmmoEngine
    from nmmo_amd.storage import DeviceExperience

    cfg = Config.preset("C4", MAP_N=4, early_stop_agent_num=8, obs_layout=abi.OBS_WIRE)
    engs = [NmmoEngine(cfg, 5, seed=12, env_index_base=5 * i) for i in range(3)]
    P, dev = engs[0].P, engs[0].device
    n = 5 * P
    assert n == 640
    for e in engs:
        e.reset()
    g = torch.Generator(device="cpu").manual_seed(9)
    steps = []
    for t in range(2):
        batch, host = [], []
        for i, e in enumerate(engs):
            e.scripted_actions(90 + t)
            e.step()
            keep = (e.mask.view(-1) != 0) & (torch.rand(n, generator=g) < 0.3).to(dev)
            lp = torch.randn(n, generator=g).to(dev)
            v = torch.randn(n, generator=g).to(dev)
            acts = torch.randint(0, 100, (n, 12), generator=g, dtype=torch.int32).to(dev)
            rew, term = e.rew.view(-1).clone(), e.term.view(-1).clone()
            sm = torch.zeros((n, 8), dtype=torch.uint8, device=dev)
            sm[:, 0:4] = rew.view(torch.uint8).view(n, 4)
            sm[:, 4] = term
            sm[:, 6] = keep.to(torch.uint8)
            st = sm.view(-1)
            w = e.obs.clone()
            flat = e.expand_obs(wire.unpack(w, 5, P)).view(n, -1).clone()
            batch.append((w, st, st[4:], st[6:], acts, lp, v, i * n))
            host.append((flat, rew, term, keep, acts, lp, v))
        steps.append((batch, host))
    sel = [[h[3].cpu().numpy() for h in host] for _, host in steps]
    tail = int(sel[1][1][512:].sum())
    assert tail >= 2, "input 1 has selected rows in its second block"
    capacity = sum(int(m.sum()) for m in sel[0]) + int(sel[1][0].sum()) + int(sel[1][1][:512].sum()) + tail // 2
    x = DeviceExperience(capacity - 1, engs[0].obs_elems, 3 * n, device=dev, record_arena_bytes=64 << 20)
    ref = ReferenceStorage(capacity - 1, engs[0].obs_elems)
    agents = []
    for t, (batch, host) in enumerate(steps):
        x.store_many(batch, t, engs[0], field_stride=8)
        cat = [torch.cat([h[k] for h in host]).cpu().numpy() for k in range(7)]
        kept = ref.store(cat[0], cat[1], cat[2], cat[3], cat[4], cat[5], cat[6], np.arange(3 * n), t)
        agents.append(np.flatnonzero(cat[3])[:kept] % n)
        assert x.ptr == ref.ptr, f"step {t}: ptr {x.ptr} != {ref.ptr}"
    k = ref.ptr
    assert k == capacity and x.status == 0
    cut = np.flatnonzero(np.concatenate(sel[1]))[len(agents[1])]  # the first selected row without room
    assert cut // n == 1 and cut % n >= 512, "the cut falls in the second block of input 1"
    for name in FIELDS[1:]:
        _same(getattr(x, name), getattr(ref, name), name)
    _same(x.env_id[:k].long(), np.array([key[0] for key in ref.sort_keys], dtype=np.int64), "env_id")
    _same(x.step[:k].long(), np.array([key[1] for key in ref.sort_keys], dtype=np.int64), "step")
    _same(x.row_agent[:k].long(), np.concatenate(agents).astype(np.int64), "row_agent")
    _same(x.gather_obs(torch.arange(k, dtype=torch.int32, device=dev)), ref.obs[:k], "gathered obs")
    _same(x.sort().long(), torch.tensor(ref.sort(), dtype=torch.int64), "sorted idxs")
    for e in engs:
        e.close()
