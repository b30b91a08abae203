"""The obs, wire and market kernels at saturation and threshold states on MI355X, bit-exact against
the CPU oracle (tests/obs_scenarios.py builds the states; tests/test_obs_scenarios.py shows on the
CPU that they reach the counts claimed). Four handles over the same 2 envs -- flat tracked, flat
under NMMO_OBS_REZERO=1, native, wire -- walk the transition schedule by set_state + observe, so
every state is written over the previous one's rows: listings above the 256 threads of a workgroup
and the 256 staged ones, the Buy-only chunk loop to chunk 16 and the chunk-17 word, the chunk-1
split at 24 entries, the 100-row Entity cut, odd nv, zero runs down to older, larger thresholds,
agents leaving the realm right after a full row, the 348-bit mask stream, wire buffers with the
largest records and the full listing block, the rebuild of all 1,024 Buy entries, the market list
of set_state and of the tick with more priced items than Market rows, and the expand-on-store paths
on full rows.

Which assertion fails when a path writes a wrong value (schedule steps count from 0, env 0's listing
counts are 0, 1024, 257, 256, 25, 24, 24, 24, 0, 961, 960, 1536, 1260, 1536, 1 and env 1's 1023, 255,
89, 88, 961, 1, 1, 1536, 1260, 1536, 0, 960, 1024, 257, 25); the ones marked * were tried by
changing that line's value in a scratch build, the walk then failed where said:
  flat_obs.hip listings past the 256 threads (the mpo loop): "tracked flat vs oracle", Buy entries
    >= 256, step 0 (env 1, 1,023 listings) and step 1 (env 0, 0 -> 1,024);
  * listings past the 256 staged ones: the same check, Market rows >= 256, at every step with more
    than 256 listings, first at step 0 (env 1), and row 256 alone at step 2 (env 0, 257), not at
    step 3 (256);
  * buy17 and the Buy-only chunk loop: Buy entries 984..1023 at step 0 (env 1, 1,023) and step 9
    (env 0, 0 -> 961), cleared again at step 10 (961 -> 960); the chunk-1 split at steps 4 -> 5 (25 -> 24)
    and the last chunk written at steps 2 -> 3 of env 1 (89 -> 88: Buy entry 88 is chunk 3's first);
  * the 100-row cut, odd nv and the Entity zero run: Entity section at step 0 (env 0, 136 in
    window), step 4 (crowd 99) and step 1 (crowd 128 -> 1: rows 5..99 must be zeroed again);
  * shrinking Market tails: Market section at step 2 (env 0, 1,024 -> 257); an agent leaving right
    after a full row: steps 11 -> 12 (env 0) and 7 -> 8 (env 1), also against the full-write handle in
    the scribble test;
  * rebuild_dep_kernel's list and cap: the wire totals and every layout's Market / Buy at step 1
    (env 0, 1,024) and step 11 (1,536 priced); the tick's own list: test_ticks_from_saturation,
    whose first ticks end with more than 1,024 priced items and later ones with fewer (asserted);
  * wire_obs.hip's long mask stream: "wire layout vs pack(native)" and "expand_obs(unpack(wire))
    vs oracle" (Attack / Give / GiveGold targets) at every step, 348 bits at steps 7..9 and 11..13;
  the wire bound: `total <= bound` before each observe, the largest record and the full listing
    block at the saturated steps (the largest buffer still has agents at the block's edge with nv <
    100, so it stays under nmmo_wire_max_bytes);
  nmmo_wire_unpack's 1,024 Buy entries: "unpack(wire) vs native" at steps 1, 7..9, 11..13;
  expand_kernel, wire_expand_kernel, record_gather_kernel: test_stores_of_full_rows."""

import functools

import numpy as np
import pytest
import torch

from nmmo_amd import abi, layout
from oracle import wire as owire
from oracle.oracle import split_state
from tests import obs_scenarios as sc
from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

N = sc.N_ENVS
LAY = layout.flat_layout()


def _engine(lay, P=128, NPC=256):
    from nmmo_amd.engine import NmmoEngine

    eng = NmmoEngine(sc.config(P, NPC, obs_layout=lay), N, seed=3)
    sc.set_tasks(eng, P)
    return eng


def _flat_pair(monkeypatch, P=128, NPC=256):
    a = _engine(abi.OBS_FLAT, P, NPC)
    monkeypatch.setenv("NMMO_OBS_REZERO", "1")
    b = _engine(abi.OBS_FLAT, P, NPC)
    monkeypatch.delenv("NMMO_OBS_REZERO")
    return a, b


def _oracle_rows(orc, dev):
    return torch.from_numpy(np.stack([orc.flat_obs(e) for e in range(N)])).to(dev)


def _sections(ks):
    """Flat-row entries -> {section: differing entries} in layout order."""
    keys = [k for k in LAY if k != "__total__"]
    offs = np.array([LAY[k].offset for k in keys])
    idx = np.searchsorted(offs, ks, side="right") - 1
    return {keys[i]: int((idx == i).sum()) for i in np.unique(idx)}


def _same(got, want, what, errs=None):
    """Bit equality of two [N, P, elems] float32 device tensors. A difference raises (or is appended
    to errs) with the sections that differ and the first differing entries."""
    got = got.reshape(want.shape)
    g, w = got.view(torch.int32), want.view(torch.int32)
    if torch.equal(g, w):
        return
    bad = torch.nonzero(g != w).cpu().numpy()
    first = [(int(e), int(a), int(k), float(got[e, a, k]), float(want[e, a, k])) for e, a, k in bad[:4]]
    msg = (f"{what}: {bad.shape[0]} entries differ in {_sections(bad[:, 2])}, envs {sorted(set(bad[:, 0].tolist()))}; "
           f"first (env, agent, entry, got, want): {first}")
    if errs is None:
        raise AssertionError(msg)
    errs.append(msg)


def _gold(blob, P=128, S=384):
    return split_state(blob, N, S, P)["ent"][:, abi.F["gold"], :P]


def _alive(blob, dev, P=128, S=384):
    a = split_state(blob, N, S, P)["ent"][:, abi.F["alive"], :P] != 0
    return torch.from_numpy(a.reshape(-1).astype(np.uint8)).to(dev)


def test_schedule_walk_every_layout(monkeypatch):
    from nmmo_amd import wire

    P = 128
    flat, rez = _flat_pair(monkeypatch)
    nat, wir = _engine(abi.OBS_NATIVE), _engine(abi.OBS_WIRE)
    orc = sc.make_oracle(sc.config())
    dev = flat.device
    bound = wire.max_bytes(N, P)
    assert bound == sc.wire_max_bytes(N, P) and wir.obs.numel() >= bound
    rec_full = owire.record_bytes(0x8000 | 100 | 12 << 7)
    back = torch.empty((N, abi.native_env_bytes(P)), dtype=torch.uint8, device=dev)
    expd = torch.empty((N, P, flat.obs_elems), dtype=torch.float32, device=dev)
    packed = torch.empty(bound, dtype=torch.uint8, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    saw_full, errs = False, []  # every state is walked; the differences are reported together

    def check(ok, what):
        if not ok:
            errs.append(what)

    for name, blob in sc.schedule():
        # the wire buffer's size from the blob alone, inside the bound before the GPU writes it
        total, rec_max, nms = sc.wire_expect(blob)
        assert total <= bound, (name, total, bound)
        orc.set_state(blob)
        for h in (flat, rez, nat, wir):
            h.set_state(blob)
            h.observe()
        want = _oracle_rows(orc, dev)
        _same(flat.obs, want, f"{name}: tracked flat vs oracle", errs)
        _same(rez.obs, want, f"{name}: rezero flat vs oracle", errs)
        # native: expand-on-demand, and the wire codec on it
        expd.fill_(float("nan"))
        _same(nat.expand_obs(out=expd), want, f"{name}: expand_obs(native) vs oracle", errs)
        packed.fill_(0x5A)
        wire.pack(nat, out=packed)
        ref = owire.pack(nat.obs.cpu().numpy(), P, _gold(blob))
        sizes = (wire.total_bytes(packed), wire.total_bytes(wir.obs), ref.nbytes)
        check(sizes == (total,) * 3, f"{name}: wire totals (pack, wire layout, oracle.wire.pack) {sizes} != {total}")
        if sizes != (total,) * 3:
            continue
        check(np.array_equal(packed[:total].cpu().numpy(), ref), f"{name}: nmmo_wire_pack vs oracle.wire.pack")
        tot = torch.tensor([total], dtype=torch.int64, device=dev)
        wire.check_buffer(packed, N, P, st, tot)
        # the wire layout: the same bytes straight from the state, decoded back to the native obs
        check(torch.equal(wir.obs[:total], packed[:total]), f"{name}: wire layout vs pack(native)")
        wire.check_buffer(wir.obs, N, P, st, tot)
        check(int(st.item()) == 0, f"{name}: nmmo_wire_check bits {int(st.item())}")
        st.zero_()
        back.fill_(0x5A)
        wire.unpack(wir.obs, N, P, out=back)
        check(torch.equal(back, nat.obs), f"{name}: unpack(wire) vs native")
        expd.fill_(float("nan"))
        _same(wir.expand_obs(back, out=expd), want, f"{name}: expand_obs(unpack(wire)) vs oracle", errs)
        if rec_max == rec_full and 1024 in nms:  # the largest records and the full listing block
            saw_full = True
            cnt = wir.obs[8 + 8 * N:8 + 8 * N + 2 * N * P].view(torch.int16).cpu().numpy().view(np.uint16)
            check((cnt == (0x8000 | 100 | 12 << 7)).any(), f"{name}: no count word of a full record")
        # an untracked buffer gets every row in full (obs_kernel), zero rows included
        out = torch.full((N, P, flat.obs_elems), float("nan"), dtype=torch.float32, device=dev)
        flat.observe(out=out)
        check(not bool(torch.isnan(out).any()), f"{name}: the full write left a NaN")
        _same(out, want, f"{name}: untracked full write vs oracle", errs)
        for h in (flat, rez, nat, wir):
            assert h.get_fault() == 0, name
    assert not errs, "\n".join(errs)
    assert saw_full
    for h in (flat, rez, nat, wir):
        h.close()


def test_repeated_state_stores_less():
    """The second observe() of an unchanged state leaves the buffer byte-identical and stores
    strictly fewer bytes than the first; the flat rows store less than a quarter of a full write."""
    sched = sc.schedule()
    before, blob = sched[sc.REPEAT[0] - 1][1], sched[sc.REPEAT[0]][1]
    assert np.array_equal(blob, sched[sc.REPEAT[1]][1])
    for lay in (abi.OBS_FLAT, abi.OBS_NATIVE):
        eng = _engine(lay)
        rows = torch.zeros((N, 2), dtype=torch.int64, device=eng.device)
        eng.set_state(before)
        eng.observe()
        eng.set_obs_counter(rows)
        eng.set_state(blob)
        eng.observe()
        first = int(rows[:, 1].sum().item())
        snap = eng.obs.clone()
        eng.set_state(blob)
        eng.observe()
        second = int(rows[:, 1].sum().item()) - first
        assert torch.equal(eng.obs.view(torch.uint8), snap.view(torch.uint8)), lay
        assert 0 < second < first, (lay, first, second)
        if lay == abi.OBS_FLAT:
            assert second < N * eng.P * eng.obs_elems * 4 // 4, second
        assert eng.get_fault() == 0
        eng.close()


def test_scribble_in_a_zero_row_is_repaired_after_tile_invalidate(monkeypatch):
    """After the saturated state, a consumer's write into the Tile section of a row that has just
    left the realm is re-zeroed once the Tile sections are invalidated."""
    flat, rez = _flat_pair(monkeypatch)
    sched = sc.schedule()
    i_sat, i_out, _ = sc.SAT_STEPS[0]
    for i in (i_sat, i_out):
        for h in (flat, rez):
            h.set_state(sched[i][1])
            h.observe()
    tile = LAY["Tile"]
    a = sc.GROUP_OUT[3]
    assert not bool(flat.obs[0, a].any())
    flat.obs[0, a, tile.offset:tile.offset + 675] = 7.0
    flat.obs_invalidate_sections(abi.OBS_SEC_TILE)
    flat.observe()
    rez.observe()
    _same(flat.obs, rez.obs.clone(), "tracked vs rezero after the Tile invalidate")
    assert flat.get_fault() == 0 and rez.get_fault() == 0
    flat.close()
    rez.close()


def test_ticks_from_saturation():
    """8 ticks of scripted actions from the saturated blob: the tick's own end-of-tick market list
    starts above 1,024 priced items and falls through the cap as listings expire."""
    from tests.test_gpu_parity import _cmp_events, _cmp_state

    blob, _ = sc.saturated_pair(128, 256, sc.GROUP_OUT)
    eng = _engine(abi.OBS_FLAT)
    orc = sc.make_oracle(sc.config())
    eng.set_state(blob)
    orc.set_state(blob)
    far_buys, priced = 0, [1536]
    for t in range(8):
        acts = orc.scripted_actions(700 + t)
        g_acts = eng.scripted_actions(700 + t)
        assert np.array_equal(g_acts.cpu().numpy(), acts), f"policy differs at tick {t}"
        buy = acts[..., layout.HEAD["Buy.MarketItem"]]
        far_buys += int(((buy >= 256) & (buy < 1024)).sum())
        orc.step(acts)
        eng.step(torch.from_numpy(acts).to(eng.device))
        torch.cuda.synchronize()
        _cmp_state(eng.get_state(), orc.get_state(), N, eng.S, f"tick {t}")
        for name in ("rew", "term", "trunc", "mask"):
            assert np.array_equal(getattr(eng, name).cpu().numpy(), getattr(orc, name)), f"{name} @ {t}"
        _cmp_events(eng, orc, N, f"tick {t}")
        _same(eng.obs, torch.from_numpy(orc.obs).to(eng.device), f"obs at tick {t}")
        d = split_state(orc.get_state(), N, orc.S, orc.P)
        priced.append(len(sc.priced_rows(d, 0, orc.P)[0]))
    assert far_buys > 0, "no Buy chose a listing index >= 256"
    assert priced[1] > 1024 and min(priced) < 1024, priced  # at and above the cap, then below
    assert priced[-1] < priced[0], "no listing was sold or delisted"
    assert eng.get_fault() == 0
    eng.close()


def test_stores_of_full_rows():
    """The saturated step stored into a DeviceExperience from each layout -- flat rows, native with
    expand-on-store, wire with decode-on-store, wire records expanded per gather -- holds the same
    observations."""
    from nmmo_amd.storage import DeviceExperience

    sched = sc.schedule()
    engs = {k: _engine(lay) for k, lay in (("flat", abi.OBS_FLAT), ("native", abi.OBS_NATIVE), ("wire", abi.OBS_WIRE))}
    dev = engs["flat"].device
    P, elems = 128, engs["flat"].obs_elems
    xs = {k: DeviceExperience(2 * N * P, elems, N * P, device=dev) for k in engs}
    xs["records"] = DeviceExperience(2 * N * P, elems, N * P, device=dev, record_arena_bytes=8 << 20)
    z = torch.zeros(N * P, device=dev)
    acts = torch.zeros((N * P, 12), dtype=torch.int32, device=dev)
    for step, i in enumerate(sc.SAT_STEPS[0][:2]):  # env 0 saturated, then its full group out
        blob = sched[i][1]
        m = _alive(blob, dev)
        for k, e in engs.items():
            e.set_state(blob)
            e.observe()
        for k, x in xs.items():
            e = engs["wire" if k == "records" else k]
            x.store(e.obs, z, z.to(torch.uint8), m, acts, z, z, step=step, engine=None if k == "flat" else e)
    torch.cuda.synchronize()
    k = xs["flat"].ptr
    state = {n: (x.ptr, x.status) for n, x in xs.items()}
    assert k > N * P and all(v == (k, 0) for v in state.values()), state
    want = xs["flat"].obs[:k]
    for name in ("native", "wire"):
        assert torch.equal(xs[name].obs[:k].view(torch.int32), want.view(torch.int32)), name
    got = xs["records"].gather_obs(torch.arange(k, dtype=torch.int32, device=dev))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "records"
    for e in engs.values():
        assert e.get_fault() == 0
        e.close()


_odd_pair = functools.lru_cache(None)(sc.saturated_pair)  # (the blobs are only read)
# The slot counts that are no multiple of 8 (flat_obs_kernel<*, 0, false>: the Entity columns staged
# element by element): (13, 4), S = 17, one partial obs group per env; (100, 50), S = 150, a partial
# last group, seven workgroups per env and three datastore-row words per lane.
UNALIGNED = [(13, 4, (1, 5, 9, 12)), (100, 50, tuple(range(16, 32)) + tuple(range(96, 100)))]


# (13, 3): S = 16 is a multiple of 8 (flat_obs_kernel<*, 0>) with one partial group
@pytest.mark.parametrize("P,NPC,out", [UNALIGNED[1], (13, 3, (1, 5, 9, 12)), UNALIGNED[0]])
def test_saturated_and_shrink_at_odd_sizes(P, NPC, out, monkeypatch):
    """S != 384, a partial last obs group, and slot counts that are no multiple of 8: saturated, the
    group out of the realm, saturated again -- flat (tracked and under NMMO_OBS_REZERO) vs the oracle."""
    sat, shrunk = _odd_pair(P, NPC, out)
    flat, rez = _flat_pair(monkeypatch, P, NPC)
    orc = sc.make_oracle(sc.config(P, NPC))
    for name, blob in (("saturated", sat), ("shrunk", shrunk), ("back", sat)):
        orc.set_state(blob)
        want = _oracle_rows(orc, flat.device)
        for h in (flat, rez):
            h.set_state(blob)
            h.observe()
            _same(h.obs, want, f"P={P} N={NPC} {name}")
            assert h.get_fault() == 0
    flat.close()
    rez.close()


@pytest.mark.parametrize("P,NPC,out", UNALIGNED)
def test_repeated_state_stores_less_at_unaligned_slot_counts(P, NPC, out):
    """test_repeated_state_stores_less's flat half where S is no multiple of 8: the second observe()
    of an unchanged state leaves the buffer byte-identical and stores strictly fewer bytes than the
    first (which zeroes the rows of `out`), so the incremental kernel serves these shapes."""
    before, blob = _odd_pair(P, NPC, out)
    eng = _engine(abi.OBS_FLAT, P, NPC)
    rows = torch.zeros((N, 2), dtype=torch.int64, device=eng.device)
    eng.set_state(before)
    eng.observe()
    eng.set_obs_counter(rows)
    eng.set_state(blob)
    eng.observe()
    first = int(rows[:, 1].sum().item())
    snap = eng.obs.clone()
    eng.set_state(blob)
    eng.observe()
    second = int(rows[:, 1].sum().item()) - first
    print(f"P={P} NPC={NPC}: first {first} B, second {second} B, full write {N * P * eng.obs_elems * 4} B")
    assert torch.equal(eng.obs.view(torch.uint8), snap.view(torch.uint8))
    assert 0 < second < first, (first, second)
    assert eng.get_fault() == 0
    eng.close()


@pytest.mark.parametrize("P,NPC,out", UNALIGNED)
def test_tile_invalidate_repairs_scribbles_at_unaligned_slot_counts(P, NPC, out, monkeypatch):
    """test_scribble_in_a_zero_row_is_repaired_after_tile_invalidate where S is no multiple of 8, on
    a row that has just left the realm and on one still in it: after the Tile sections are
    invalidated the tracked buffer equals the NMMO_OBS_REZERO handle's and the oracle's rows."""
    sat, shrunk = _odd_pair(P, NPC, out)
    flat, rez = _flat_pair(monkeypatch, P, NPC)
    for blob in (sat, shrunk):
        for h in (flat, rez):
            h.set_state(blob)
            h.observe()
    alive = split_state(shrunk, N, P + NPC, P)["ent"][0, abi.F["alive"], :P] != 0
    a_out, a_in = out[-1], next(a for a in range(P) if alive[a] and a not in out)
    assert not alive[a_out] and not bool(flat.obs[0, a_out].any()) and bool(flat.obs[0, a_in].any())
    tile = LAY["Tile"]
    for a in (a_out, a_in):
        flat.obs[0, a, tile.offset:tile.offset + 675] = 7.0
    flat.obs_invalidate_sections(abi.OBS_SEC_TILE)
    flat.observe()
    rez.observe()
    _same(flat.obs, rez.obs.clone(), f"P={P} N={NPC}: tracked vs rezero after the Tile invalidate")
    orc = sc.make_oracle(sc.config(P, NPC))
    orc.set_state(shrunk)
    _same(flat.obs, _oracle_rows(orc, flat.device), f"P={P} N={NPC}: tracked vs oracle after the Tile invalidate")
    assert flat.get_fault() == 0 and rez.get_fault() == 0
    flat.close()
    rez.close()
