"""The wrapper cases (tests/wrapper_cases.py) on the CPU alone: every case reaches what it claims
(its witness holds on the expectation), the reference functions handle every row set, the
expectation is consistent with itself (the bitset is the tuple set, the count the whole-log count,
the records of a final step equal process_event_log over the agent's rows), and the inject_events
hook of the CPU stepper puts rows where the tick would. The selections of contended tick scenarios
that tests/test_gpu_wrapper_states.py runs with the wrapper on are driven here through the oracle
env and the oracle wrapper alone, with their witnesses. The GPU counterpart is
tests/test_gpu_wrapper_states.py. CPU only."""

import ctypes

import numpy as np
import pytest

from nmmo_amd import abi
from oracle.wrapper import count_unique_events, process_event_log
from tests import wrapper_cases as wc

N = wc.N_ENVS
CASES = wc.cases()


@pytest.mark.parametrize("cid", [c[0] for c in CASES])
def test_case_reaches_its_witness(cid):
    case = wc.build(cid)
    snaps = wc.expectation(case)
    assert len(snaps) == len(case.batches)
    case.witness(snaps)
    P = case.P
    s = snaps[-1]
    for e in range(N):  # the per-step bookkeeping equals one pass over everything walked
        rows = np.concatenate([x.walked[e] for x in snaps])
        if case.name == "W6" and e == 0:  # reset in the last step: nothing walked since
            rows = wc.EMPTY
        for a in range(1, P + 1):
            own = rows[rows[:, 1] == a]
            seen = set()
            n = count_unique_events(wc.countable(own), seen)
            assert s.state["curr_count"][e, a - 1] == n, (cid, e, a)
            assert np.array_equal(s.uniq[e, a - 1], wc.bitset(seen)), (cid, e, a)
            assert int(np.unpackbits(s.uniq[e, a - 1].view(np.uint8)).sum()) == len({t for t in seen if wc.in_range(*t)})
            if all(wc.in_range(*t) for t in seen):
                assert n == process_event_log(own)[0]["achieved/unique_events"]


@pytest.mark.parametrize("sel", wc.SCENARIOS, ids=[s[0] for s in wc.SCENARIOS])
def test_scenario_selection_reaches_its_witnesses(sel):
    """The tick scenarios chosen for the wrapper reach what they were chosen for, on the oracle env
    and the oracle wrapper alone; what OracleWrapper holds is consistent with `Model`'s restatement."""
    cid, builder, P, NPC, preset, agent, kw, wit = sel
    seen = []

    def on_tick(t, ticks, orc, ow, a, dropped):
        st, uq = wc.oracle_state(ow)
        seen.append((int(st["curr_count"].sum()), int(uq.any(axis=2).sum())))
        assert np.all(st["curr_count"] >= st["prev_count"])

    reached = wc.oracle_walk(builder, P, NPC, preset, agent, kw, on_tick)
    assert set(wit) <= reached, f"{cid}: witnesses not reached: {sorted(set(wit) - reached)}"
    assert seen and seen[0][0] > 0 and seen[0][1] > 0, "the first tick logged nothing for the wrapper"


def test_saturated_state_reaches_the_obs_edits():
    """The saturated pair with NPC types 1, 2, 3: full windows hold all three, the dangerous-NPC edit
    clears some Attack.Target bits and keeps others, disable_give changes the Give masks; both
    states are valid blobs the oracle takes."""
    from nmmo_amd.layout import flat_layout
    from tests import obs_scenarios as sc

    orc = sc.make_oracle(sc.config())
    lay = flat_layout()
    for i, blob in enumerate(wc.saturated_npcs()):
        orc.set_state(blob)
        assert np.array_equal(orc.get_state(), blob)
        raw, edited = wc.edited_obs(orc, wc.YAO, {})
        if i == 0:
            full, cleared, kept = wc.obs_edit_witness(raw, edited, lay)
            assert full >= 4 and cleared >= 10 and kept > 1000
        segs = [lay["ActionTargets." + k] for k in ("Give.InventoryItem", "Give.Target", "GiveGold.Target", "GiveGold.Price")]
        assert any(np.any(raw[:, :, s.offset:s.offset + s.shape[0]] != edited[:, :, s.offset:s.offset + s.shape[0]]) for s in segs)


def test_bit_formula_and_edges():
    assert wc.bit_index(*wc.tuple_of_bit(4895)) == 4895 and wc.tuple_of_bit(4895) == (91, 17, 15)
    assert wc.tuple_of_bit(31) == (1, 1, 15) and wc.tuple_of_bit(32) == (1, 2, 0)
    assert [wc.bit_index(c, 0, 0) for c in wc.CODES] == [288 * i for i in range(17)]
    w = wc.bitset({wc.tuple_of_bit(b) for b in wc.EDGE_BITS} | {(99, 0, 0), (1, 18, 0), (1, 0, 16), (1, -1, 0)})
    assert [int(x) for x in np.flatnonzero(w)] == [0, 1, 2, 152] and w[152] == 1 << 31 and w[0] == 1 << 31
    assert abi.UNIQ_WORDS * 32 == 17 * 18 * 16


def test_w5_records_equal_the_whole_log_scan():
    for cid in ("W5-eval0", "W5-eval1"):
        case = wc.build(cid)
        snaps = wc.expectation(case)
        for e in range(N):
            rows = np.concatenate([x.walked[e] for x in snaps])
            for a, info in snaps[-1].infos[e].items():
                ach, perf = process_event_log(rows[rows[:, 1] == a])
                for k, v in list(ach.items()) + list(perf.items()):
                    assert info["stats"][k] == float(v)
                assert info["length"] == case.cfg.HORIZON
                if case.eval_mode:
                    assert info["return"] == info["curriculum"]["task"][0]


@pytest.mark.parametrize("cap", [64, 100])
def test_inject_events_of_the_cpu_stepper(cap):
    """nmmo_inject_events through the CPU library's C-ABI: ring placement, the count, more rows
    than the ring holds, and the argument errors."""
    from nmmo_amd import _native
    from nmmo_amd.config import Config
    from tests.test_cpu_abi import CPU_LIB
    from oracle import oracle

    oracle.build()
    cpu = _native.declare(ctypes.CDLL(CPU_LIB))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for ec in (cap, 0):
        c = Config.preset("C2", MAP_N=2, PLAYER_N=4, event_cap=ec).to_c()
        h = ctypes.c_void_p()
        assert cpu.nmmo_create(ctypes.byref(c), 2, 1, 0, None, ctypes.byref(h)) == 0
        rows = np.arange(9 * (cap + 37), dtype=np.int32).reshape(-1, 9)
        if ec == 0:
            assert cpu.nmmo_inject_events(h, 0, p(rows), 3) == abi.NMMO_E_INVALID
            cpu.nmmo_destroy(h)
            continue
        assert cpu.nmmo_inject_events(None, 0, p(rows), 3) == abi.NMMO_E_INVALID
        assert cpu.nmmo_inject_events(h, 0, None, 3) == abi.NMMO_E_INVALID
        assert cpu.nmmo_inject_events(h, 2, p(rows), 3) == abi.NMMO_E_INVALID
        assert cpu.nmmo_inject_events(h, -1, p(rows), 3) == abi.NMMO_E_INVALID
        assert cpu.nmmo_inject_events(h, 1, p(rows), -1) == abi.NMMO_E_INVALID
        got, k = np.zeros((cap, 9), np.int32), ctypes.c_int32()
        assert cpu.nmmo_inject_events(h, 1, p(rows), 10) == 0
        assert cpu.nmmo_get_events(h, 1, p(got), cap, ctypes.byref(k)) == 0 and k.value == 10
        assert np.array_equal(got[:10], rows[:10])
        assert cpu.nmmo_inject_events(h, 1, p(rows), cap + 37) == 0
        assert cpu.nmmo_get_events(h, 1, p(got), cap, ctypes.byref(k)) == 0 and k.value == cap
        assert np.array_equal(got, rows[37:cap + 37])
        assert cpu.nmmo_get_events(h, 0, p(got), cap, ctypes.byref(k)) == 0 and k.value == 0
        cpu.nmmo_destroy(h)
