"""The wrapper pass (csrc/wrap.hip, SPEC.md §13) on built event rows and contended tick states on
MI355X, bit-exact against the reference's own functions (tests/wrapper_cases.py builds the cases and
their expectations with oracle/wrapper.py's count_unique_events / process_event_log / OracleWrapper;
tests/test_wrapper_cases.py shows on the CPU that every case reaches its witness). Nothing here has a
tolerance: counts, bitset words, accumulators, double returns, float32 rewards, records and obs are
compared for equality, and the fault word stays 0 (every row set and state is legal input).

  test_synthetic_rows: W1-W6 and WP through NmmoEngine.inject_events + no-op steps; after every
    step the event log, every NmmoWrapState field, the `experienced` words of every agent of both
    envs, the shaped rewards, the records and the dropped-row counter equal the expectation.
  test_tick_scenario_with_wrapper: tests/tick_scenarios.py's states (and D1, equipped armor) with
    the wrapper on against OracleEnvs + OracleWrapper, after every tick; flat obs after the first
    and the last tick.
  test_set_state_twice_with_the_wrapper_on: B3, A1, B3 on one engine, each walk against a fresh
    OracleWrapper. Before nmmo_set_state re-initialised the wrapper layer this failed at "A1 after
    B3 tick 0" (the cursor stayed at B3's event count, A1's rows were never walked, B3's bitsets
    and accumulators carried over).
  test_obs_edits_at_saturation: the wrappers' obs edits on the saturated pair of
    tests/obs_scenarios.py in the flat (tracked, foreign buffer), native and wire layouts.

Which test fails when a line of wrap.hip is wrong. Each mutation was made in a scratch copy of the
kernel and linked into a library of its own; the tests named failed on MI355X with that library
and pass with the tree's, except the one marked untried:
  atomicOr -> plain read-modify-write of the word: W1 "curr_count" (73 for 72), W2-128 / W2-100
    "curr_count" (2 or 3 for the one tuple logged three times), W6, A4-yaofeng and A4-kit
    "experienced words" (bits of other tuples in the same word lost to the race).
  b >> 5 -> b >> 6: every test but the obs edits and the hook's arguments, first W1 "curr_count" / "experienced words" (bit 32 lands
    in word 0, tuples 32 bits apart collide).
  the `ag >= P` check removed: untried on the GPU, on purpose. W3's row of ent_id P + 1 in env 0
    would set a bit of env 1's agent 0, which W3's comparison of every word of both envs reports
    ("experienced words"), but W3's ent_id 2^31 - 1 row would index far outside the allocation in
    the same build, and no test here may write out of bounds.
  i % cap -> i & (cap - 1): W4-cap100 "curr_count" (rows read from other ring slots) and
    M2_cap100-kit "shaped reward"; W4-cap64 and M2_cap64-kit pass, as they must.
  lo = evc - cap dropped: W4-cap64 and W4-cap100 step 2 "curr_count" (the overwritten rows' slots are
    walked a second time: their PLAYER_KILL / EARN_GOLD rows count double).
  min(clip, ...) dropped: W2 "shaped reward" (6.19 for 0.20: 602 new counts), W1, W3, W5, W6, A4-kit,
    A5-kit and B2-kit "shaped reward".
  the vector clear taken whatever P * 153 % 4 is (the alignment test kept, so that no misaligned
    store is issued): W6 step 1 "experienced words" at (env 0, agent 2, word 152): the three tail
    words of env 0 are not cleared.
  nmmo_set_state without the wrapper re-initialisation (the parent commit's): only
    test_set_state_twice_with_the_wrapper_on fails, at "A1 after B3 tick 0: shaped reward" (no
    explore bonus: the walk saw no rows).
"""

import ctypes

import numpy as np
import pytest
import torch

from nmmo_amd import abi
from nmmo_amd.wrappers import infos_from_records, wrapper_config
from tests import obs_scenarios as sc
from tests import tick_scenarios as ts
from tests import wrapper_cases as wc
from tests.conftest import gpu_available
from tests.test_gpu_parity import _cmp_events
from tests.test_gpu_wrapper import _eq_info

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

N = wc.N_ENVS


def _engine(cfg, agent, kw, seed=3, tasks=True):
    from nmmo_amd.engine import NmmoEngine

    eng = NmmoEngine(cfg, N, seed=seed)
    if tasks:
        sc.set_tasks(eng, cfg.PLAYER_N)
    eng.set_wrapper(wrapper_config(agent, **kw))
    return eng


def _dev(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _same_state(eng, want, want_uq, where):
    st, uq = eng.wrapper_state()
    for name in st.dtype.names:
        if not np.array_equal(st[name], want[name]):
            bad = np.argwhere(st[name] != want[name])[:4]
            raise AssertionError(f"{where}: {name} differs at (env, agent, ..) {bad.tolist()}: gpu "
                                 f"{[st[name][tuple(b)].tolist() for b in bad]} want {[want[name][tuple(b)].tolist() for b in bad]}")
    if not np.array_equal(uq, want_uq):  # every word of every agent of both envs, the last one included
        bad = np.argwhere(uq != want_uq)[:4]
        raise AssertionError(f"{where}: experienced words differ at (env, agent, word) {bad.tolist()}: gpu "
                             f"{[hex(uq[tuple(b)]) for b in bad]} want {[hex(want_uq[tuple(b)]) for b in bad]}")


def _same_outputs(eng, rew, term, trunc, mask, envs, where):
    g = eng.rew.cpu().numpy()
    for e in envs:
        if not np.array_equal(g[e].view(np.int32), rew[e].view(np.int32)):
            bad = np.flatnonzero(g[e] != rew[e])[:4]
            raise AssertionError(f"{where}: env {e} shaped reward differs at agents {bad.tolist()}: gpu "
                                 f"{g[e][bad].tolist()} want {rew[e][bad].tolist()}")
        for name, w in (("term", term), ("trunc", trunc), ("mask", mask)):
            assert np.array_equal(getattr(eng, name).cpu().numpy()[e], w[e]), f"{where}: env {e} {name}"


@pytest.mark.parametrize("cid", [c[0] for c in wc.cases()])
def test_synthetic_rows(cid):
    case = wc.build(cid)
    snaps = wc.expectation(case)
    eng = _engine(case.cfg, wc.AGENT, dict(wc.AGENT_KW, eval_mode=case.eval_mode), seed=wc.SEED, tasks=False)
    case.prepare(eng)
    acts = _dev(eng, case.actions())
    dropped0 = eng.wrapper_dropped_events()
    for t, (batch, s) in enumerate(zip(case.batches, snaps)):
        where = f"{cid} step {t}"
        for e, rows in sorted(batch.items()):
            eng.inject_events(e, rows)
        if t in case.end:
            eng.end_episodes(case.end[t])
        if t in case.only:
            eng.step_envs(torch.tensor(case.only[t], dtype=torch.int32, device=eng.device), acts)
        else:
            eng.step(acts)
        torch.cuda.synchronize()
        assert eng.get_fault() == 0, f"{where}: fault word"
        for e in range(N):
            assert np.array_equal(eng.events(e), s.events[e]), f"{where}: env {e} event log"
        _same_state(eng, s.state, s.uniq, where)
        _same_outputs(eng, s.rew, s.term, s.trunc, s.mask, s.envs, where)
        infos = infos_from_records(eng.info_records())
        for e in s.envs:
            _eq_info(infos[e], s.infos[e], f"{where} env {e}")
        assert eng.wrapper_dropped_events() - dropped0 == s.dropped, f"{where}: dropped rows"
    eng.close()


def _cmp_walk(eng, orc, ow, dropped, where):
    assert eng.get_fault() == 0, f"{where}: fault word"
    _cmp_events(eng, orc, N, where)
    _same_outputs(eng, orc.rew, orc.term, orc.trunc, orc.mask, range(N), where)
    infos = infos_from_records(eng.info_records())
    for e in range(N):
        _eq_info(infos[e], ow.infos[e], f"{where} env {e}")
    _same_state(eng, *wc.oracle_state(ow), where)
    assert eng.wrapper_dropped_events() == dropped, f"{where}: dropped rows"


def _same_obs(eng, orc, where):
    if orc.obs is None:
        return
    got = eng.obs.cpu().numpy().reshape(orc.obs.shape)
    if not np.array_equal(got.view(np.int32), orc.obs.view(np.int32)):
        bad = np.argwhere(got.view(np.int32) != orc.obs.view(np.int32))[:5]
        raise AssertionError(f"{where}: flat obs differ at (env, agent, entry) {bad.tolist()}")


def _walk(eng, orc, blob_acts, agent, kw, where, builder=None):
    eng.set_state(blob_acts[1])
    torch.cuda.synchronize()
    base = eng.wrapper_dropped_events()

    def on_tick(t, ticks, orc, ow, a, dropped):
        eng.step(_dev(eng, a))
        torch.cuda.synchronize()
        _cmp_walk(eng, orc, ow, base + dropped, f"{where} tick {t}")
        if t in (0, ticks - 1):
            _same_obs(eng, orc, f"{where} tick {t}")

    return wc.oracle_walk(builder, eng.P, eng.S - eng.P, None, agent, kw, on_tick, orc=orc, blob_acts=blob_acts)


@pytest.mark.parametrize("sel", wc.SCENARIOS, ids=[s[0] for s in wc.SCENARIOS])
def test_tick_scenario_with_wrapper(sel):
    cid, builder, P, NPC, preset, agent, kw, wit = sel
    ba = builder(P, NPC, preset)
    eng = _engine(ba[0], agent, kw)
    reached = _walk(eng, ts.make_oracle(ba[0]), ba, agent, kw, cid)
    assert set(wit) <= reached, f"{cid}: witnesses not reached: {sorted(set(wit) - reached)}"
    eng.close()


def test_set_state_twice_with_the_wrapper_on():
    """B3, then A1, then B3 again on one engine whose wrapper stays on: every walk equals a fresh
    oracle wrapper's (nmmo_set_state re-initialises the layer, SPEC §13 Reset)."""
    cfg, blob_b, acts_b, _ = ts.B3()
    _, blob_a, acts_a, _ = ts.A1()
    eng, orc = _engine(cfg, wc.KIT, wc.KIT_KW), ts.make_oracle(cfg)
    for where, blob, acts in (("B3 first", blob_b, acts_b), ("A1 after B3", blob_a, acts_a), ("B3 after A1", blob_b, acts_b)):
        _walk(eng, orc, (cfg, blob, acts[:1], None), wc.KIT, wc.KIT_KW, where)
    eng.close()


def _same_rows(got, want, where):
    got = got.reshape(want.shape)
    if not torch.equal(got.view(torch.int32), want.view(torch.int32)):
        bad = torch.nonzero(got.view(torch.int32) != want.view(torch.int32))[:5].cpu().tolist()
        raise AssertionError(f"{where}: obs differ at (env, agent, entry) {bad}")


def _obs_engines(cfg_kw, agent, kw):
    from nmmo_amd.engine import NmmoEngine

    engs = {}
    for name, lay in (("flat", abi.OBS_FLAT), ("native", abi.OBS_NATIVE), ("wire", abi.OBS_WIRE)):
        eng = NmmoEngine(sc.config(obs_layout=lay, **cfg_kw), N, seed=3)
        sc.set_tasks(eng, eng.P)
        eng.set_wrapper(wrapper_config(agent, **kw))
        engs[name] = eng
    return engs


def _check_layouts(engs, want, where):
    """Every layout's obs of the engines' current state against `want` [N, P, elems] on the device:
    the tracked flat buffer, a foreign flat buffer, native expanded, wire decoded by oracle/wire.py."""
    from oracle import wire as owire

    flat, nat, wir = engs["flat"], engs["native"], engs["wire"]
    P = flat.P
    flat.observe()
    _same_rows(flat.obs, want, f"{where}: tracked flat")
    out = torch.full((N, P, flat.obs_elems), float("nan"), dtype=torch.float32, device=flat.device)
    flat.observe(out=out)
    _same_rows(out, want, f"{where}: foreign flat buffer")
    nat.observe()
    _same_rows(nat.expand_obs(), want, f"{where}: expand_obs(native)")
    wir.observe()
    torch.cuda.synchronize()
    back = owire.unpack(wir.obs.cpu().numpy(), N, P)
    _same_rows(wir.expand_obs(torch.from_numpy(back).to(wir.device)), want, f"{where}: expand_obs(oracle.wire.unpack(wire))")
    for h in engs.values():
        assert h.get_fault() == 0, where


def test_obs_edits_at_saturation():
    """The wrappers' obs edits where the obs kernels are fullest: 100 shown entities with passive,
    neutral and hostile NPCs among them, a full market, then a group out of the realm and back.
    yaofeng's flags (disable_give, donot_attack_dangerous_npc) by set_state + observe; the start
    kit's Sell.Price[prev_price] after one step whose Sell.Price actions are non-zero."""
    from nmmo_amd.layout import flat_layout

    sat, shrunk = wc.saturated_npcs()
    orc = sc.make_oracle(sc.config())
    lay = flat_layout()
    engs = _obs_engines({}, wc.YAO, {})
    dev = engs["flat"].device
    for name, blob in (("saturated", sat), ("group out", shrunk), ("back", sat)):
        orc.set_state(blob)
        raw, edited = wc.edited_obs(orc, wc.YAO, {})
        if name == "saturated":
            wc.obs_edit_witness(raw, edited, lay)
        assert not np.array_equal(raw, edited)
        for h in engs.values():
            h.set_state(blob)
        _check_layouts(engs, torch.from_numpy(edited).to(dev), f"yaofeng {name}")
    for h in engs.values():
        h.close()
    # the start kit: one step from the saturated state, every agent with its own Sell.Price index
    engs = _obs_engines({}, wc.KIT, wc.KIT_KW)
    P = engs["flat"].P
    acts = ts.noop(P, 1)[0]
    acts[:, :, 10] = (7 * np.arange(P)[None, :] + 3 * np.arange(N)[:, None]) % 98 + 1
    orc.set_state(sat)
    orc.step(acts)
    raw, edited = wc.edited_obs(orc, wc.KIT, wc.KIT_KW, prev_price=acts[:, :, 10])
    sp = lay["ActionTargets.Sell.Price"]
    cleared = (raw[:, :, sp.offset:sp.offset + 99] != 0) & (edited[:, :, sp.offset:sp.offset + 99] == 0)
    assert cleared.sum(axis=2).max() == 1 and cleared.any(axis=2).sum() > P, "a Sell.Price entry per agent in the realm"
    assert not cleared[:, :, 0].any(), "the cleared entries are the non-zero indices the actions named"
    want = torch.from_numpy(edited).to(dev)
    for lname, h in engs.items():
        h.set_state(sat)
        h.step(_dev(h, acts))
        torch.cuda.synchronize()
        if lname == "flat":
            _same_rows(h.obs, want, "start kit: the step's own flat obs")
    _check_layouts(engs, want, "start kit after one step")
    for h in engs.values():
        h.close()


def test_inject_events_arguments():
    """nmmo_inject_events' refusals (null rows, a bad env, a negative count, no event log), the rows
    read back where the tick would have put them, and more rows than the ring holds."""
    from nmmo_amd._native import NativeError, lib
    from nmmo_amd.config import Config
    from nmmo_amd.engine import NmmoEngine

    off = NmmoEngine(Config.preset("C2", MAP_N=2, PLAYER_N=4, event_cap=0), N, seed=1)
    rows = np.arange(9 * 137, dtype=np.int32).reshape(-1, 9)
    with pytest.raises(NativeError, match="event log"):
        off.inject_events(0, rows[:3])
    off.close()
    eng = NmmoEngine(Config.preset("C2", MAP_N=2, PLAYER_N=4, event_cap=100), N, seed=1)
    eng.reset()
    p = rows.ctypes.data_as(ctypes.c_void_p)
    assert lib().nmmo_inject_events(eng.h, 0, None, 3) == abi.NMMO_E_INVALID
    assert lib().nmmo_inject_events(eng.h, N, p, 3) == abi.NMMO_E_INVALID
    assert lib().nmmo_inject_events(eng.h, -1, p, 3) == abi.NMMO_E_INVALID
    assert lib().nmmo_inject_events(eng.h, 0, p, -1) == abi.NMMO_E_INVALID
    assert len(eng.events(0)) == 0 and len(eng.events(1)) == 0
    eng.inject_events(1, rows[:10])
    assert np.array_equal(eng.events(1), rows[:10])
    eng.inject_events(1, rows)
    assert np.array_equal(eng.events(1), rows[37:]) and len(eng.events(0)) == 0
    assert eng.get_fault() == 0
    eng.close()
