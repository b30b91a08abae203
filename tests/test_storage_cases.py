"""The storage case table (tests/storage_cases.py) on the CPU, with oracle/storage.py
ReferenceStorage alone: every case has the property its name claims, so that the GPU comparison
(tests/test_gpu_storage_shapes.py) runs the block, chunk and rounding paths it is meant to run."""

import numpy as np
import pytest

from oracle.storage import ReferenceStorage
from tests import storage_cases as sc

S = sc.store_cases()
G = sc.gae_cases()
R = sc.gather_cases()
W = sc.row_width_cases()


def _replay(case):
    """-> (ref, per recv: rows kept, ptr before)."""
    ref = ReferenceStorage(case.batch_size, case.E)
    log = []
    for rv in case.recvs:
        p0 = ref.ptr
        log.append((sc.reference_store(ref, case, rv), p0))
    return ref, log


def test_store_table_covers_the_shapes():
    rows = {len(rv.mask) for c in S for rv in c.recvs}
    assert {511, 512, 513, 1024, 1537, 512 * 512 + 513} <= rows
    assert {511, 512, 513, 1024, 1025, 1537} <= {c.n_slots for c in S}
    masks = [rv.mask for c in S for rv in c.recvs]
    assert any(m.all() for m in masks) and any(not m.any() and len(m) > 512 for m in masks)
    assert any(m.sum() == 1 and m[-1] and len(m) > 3 * 512 for m in masks), "only the last row"
    assert any(len(m) >= 1024 and not m[512:1024].any() and m[:512].any() and m[1024:].any() for m in masks)
    assert any(rv.env_id is not None for c in S for rv in c.recvs) and any(rv.env_id is None for c in S for rv in c.recvs)
    for c in S:
        for rv in c.recvs + (c.second or []):
            n = len(rv.mask)
            assert rv.obs.shape == (n, c.E) and rv.obs.dtype == np.float32 and len(np.unique(rv.obs)) == n * c.E
            assert rv.actions.shape == (n, 12) and rv.actions.dtype == np.int32
            keep = sc.reference_mask(c, rv) != 0
            ids = sc.ids_of(rv)[keep]
            assert len(np.unique(ids)) == len(ids), f"{c.name}: env ids are distinct within one store"
            assert not len(ids) or (ids.min() >= 0 and ids.max() < c.n_slots), c.name
            if n > 64:
                assert set(np.unique(rv.dones)) == {0, 1}, f"{c.name}: dones of both values"
        steps = [rv.step for rv in c.recvs]
        assert steps == sorted(set(steps)), f"{c.name}: rows of an env id arrive in step order"
    assert sum(1 for c in S if c.second) >= 2


@pytest.mark.parametrize("case", S, ids=[c.name for c in S])
def test_store_cut_is_where_the_name_says(case):
    ref, log = _replay(case)
    for k, (rv, (kept, p0)) in enumerate(zip(case.recvs, log)):
        sel = np.flatnonzero(sc.reference_mask(case, rv))
        if k != case.cut_recv:
            assert kept == len(sel), f"{case.name}: recv {k} is not cut"
            continue
        assert p0 > 0, "the cut store starts at ptr0 > 0"
        assert kept < len(sel) and ref.ptr == case.batch_size + 1
        cut = int(sel[kept])  # the first selected row that finds no room
        per_block = sc.selected_per_block(rv.mask)
        assert len(per_block) >= 4 and len(set(per_block.tolist())) > 1, "per-block counts differ"
        if case.cut == "boundary":
            assert cut % sc.BLOCK == 0 and cut > 0 and rv.mask[cut - 1]
            assert per_block[:cut // sc.BLOCK].sum() == kept, "blocks 0..k hold exactly the room"
        elif case.cut == "above512":
            assert cut // sc.BLOCK > 512
        else:
            assert cut // sc.BLOCK == case.cut[1]
    if case.cut is None:
        assert case.cut_recv is None


def test_store_cuts_cover_the_rooms():
    room = {}
    for c in S:
        if c.cut_recv is not None:
            _, log = _replay(c)
            room[c.name] = log[c.cut_recv][0]
    assert room["cut_room0"] == 0 and room["cut_room1"] == 1
    assert {c.cut for c in S} >= {("block", 0), ("block", 2), "boundary", "above512"}


def test_out_of_range_case():
    (c,) = [c for c in S if c.oob]
    rv = c.recvs[-1]
    ids = rv.env_id[list(c.oob)]
    assert all(r // sc.BLOCK >= 1 and rv.mask[r] for r in c.oob)
    assert (ids >= c.n_slots).sum() == 1 and (ids < 0).sum() == 1
    assert not sc.reference_mask(c, rv)[list(c.oob)].any()


@pytest.mark.parametrize("case", S, ids=[c.name for c in S])
def test_sort_case_spans_its_chunks(case):
    """K: where n_slots has more than two chunks of 512 the stored ids have rows in three of
    them at least, so a dropped carry or a stale scan buffer moves rows."""
    ref, _ = _replay(case)
    ids = np.array([k[0] for k in ref.sort_keys], dtype=np.int64).reshape(-1)
    assert case.chunks3 == (case.n_slots > 2 * sc.BLOCK)
    if case.chunks3:
        assert len(set((ids // sc.BLOCK).tolist())) >= 3
    if len(ids) > 2 and not case.name.startswith(("cut_", "large")):
        assert ids.min() == 0 and ids.max() == case.n_slots - 1, "ids 0 and n_slots - 1 are stored"
    order = ref.sort()
    assert sorted(order) == list(range(len(ids)))


def test_sort_table_covers_sparse_and_repeated_ids():
    (c,) = [c for c in S if c.name.startswith("sparse")]
    ref, _ = _replay(c)
    cnt = np.bincount([k[0] for k in ref.sort_keys], minlength=c.n_slots)
    assert (cnt == 0).sum() > c.n_slots // 2 and cnt.max() >= 3 and cnt[0] and cnt[-1]
    assert sum(1 for c in S if c.chunks3) >= 4


def test_gae_table_covers_sizes_pairs_and_kinds():
    assert {c.B for c in G} == set(sc.GAE_SIZES)
    assert {(c.gamma, c.gae_lambda) for c in G} == set(sc.GAE_PAIRS)
    differ = [(g, l) for g, l in sc.GAE_PAIRS if np.float32(g * l) != np.float32(g) * np.float32(l)]
    assert differ, "a pair tells the double product from the float32 product"
    assert any((c.gamma, c.gae_lambda) in differ and c.B > 64 and c.kind == "normal" for c in G)
    for c in G:
        n = c.B + 1
        assert sorted(c.idxs.tolist()) == list(range(n))
        assert c.rewards.shape == c.values.shape == c.dones.shape == (n,)
        assert c.rewards.dtype == c.values.dtype == c.dones.dtype == np.float32
    for kind in ("normal", "large", "subnormal", "zeros"):
        for pair in sc.GAE_PAIRS:
            modes = {(bool(c.dones.all()), bool(c.dones.any())) for c in G
                     if c.kind == kind and (c.gamma, c.gae_lambda) == pair}
            assert kind == "normal" or modes == {(True, True), (False, True), (False, False)}, (kind, pair)
    assert any(c.kind == "large" and np.abs(c.values).max() > 1e30 for c in G)
    assert any(c.kind == "zeros" and np.signbit(c.values).any() and not np.signbit(c.values).all() for c in G)


@pytest.mark.parametrize("case", G, ids=[c.name for c in G])
def test_gae_reference_has_no_nan(case):
    """NaN sign and payload differ between the host and the GPU: no case may produce one."""
    adv = sc.gae_reference(case).numpy()
    assert adv.shape == (case.B,) and not np.isnan(adv).any()
    if case.kind == "subnormal":
        tiny = np.finfo(np.float32).tiny
        assert ((adv != 0) & (np.abs(adv) < tiny)).any(), "nonzero subnormal advantages"
        assert (np.abs(adv) < tiny).all()


def test_gather_table_covers_widths_counts_and_dtypes():
    assert {c.words for c in R} == set(sc.WIDTHS)
    assert {(c.words, len(c.idx)) for c in R if c.src.dtype == np.float32} == {(w, n) for w in sc.WIDTHS for n in sc.COUNTS}
    assert {c.src.dtype for c in R} == {np.dtype(t) for t in (np.float32, np.int32, np.int64, np.uint8)}
    for c in R:
        assert c.src[0].nbytes == 4 * c.words and c.idx.dtype == np.int32
        assert 0 <= c.idx.min() and c.idx.max() < len(c.src)
    assert any(len(set(c.idx.tolist())) < len(c.idx) for c in R), "repeats"
    assert any(len(c.idx) > 2 and (np.diff(c.idx) < 0).all() for c in R), "reversed order"
    assert all((c.idx == len(c.src) - 1).any() for c in R), "the last source row"
    assert [c.E for c in W] == sc.WIDTHS
    for c in W:
        assert all(len(rv.mask) == 5 and rv.mask.sum() == 3 for rv in c.recvs)
