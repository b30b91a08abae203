"""The tick scenarios (tests/tick_scenarios.py) on the CPU oracle alone. For every scenario and
size: set_state, step the explicit actions, then the scenario's witness and check_invariants on the
result. That shows two things: each scenario reaches the contention it claims (the "both outcomes
occur" conditions are asserted here, on the SPEC restatement of the Buy order), and the serial
oracle agrees with a restatement of SPEC.md §5, §9 and §11 that never reads the oracle's outputs.
The GPU counterpart is tests/test_gpu_tick_contention.py."""

import numpy as np
import pytest

from nmmo_amd import abi
from oracle.oracle import split_state
from tests import tick_scenarios as ts

E, F = abi.E, abi.F
N = ts.N_ENVS
CASES = ts.cases()


def _run(builder, P, NPC, preset):
    cfg, blob, acts, witness = builder(P, NPC, preset)
    orc = ts.make_oracle(cfg)
    orc.set_state(blob)
    assert np.array_equal(orc.get_state(), blob), "set_state / get_state round trip"
    outs = []

    def step(a):
        orc.step(a)
        outs.append((orc.rew.copy(), orc.term.copy(), orc.trunc.copy(), orc.mask.copy()))

    post = ts.run(step, orc.get_state, orc.events, blob, acts, P, orc.S, witness)
    return cfg, blob, acts, witness, orc, outs, post


@pytest.mark.parametrize("name,builder,P,NPC,preset", CASES, ids=[c[0] for c in CASES])
def test_scenario_on_the_oracle(name, builder, P, NPC, preset):
    cfg, blob, acts, witness, orc, outs, post = _run(builder, P, NPC, preset)
    assert acts.dtype == np.int32 and acts.shape[1:] == (N, P, 12) and 1 <= acts.shape[0] <= 6
    assert int(post["ent"][:, F["gold"], :P].max()) < 32767
    if builder is not ts.A5:
        _no_npc_decides(name, blob, post, P, orc.S)
    if hasattr(witness, "outputs"):
        assert witness.outputs(*outs[0]), f"{name}: rew / term / trunc / mask of the first tick"
    if getattr(witness, "auto_reset", False):  # M1: checked here on the oracle
        env = post["env"]
        assert np.all(env[:, E["episode"]] == 1) and np.all(env[:, E["tick"]] == 0) and not env[:, E["done"]].any()
        assert np.all(env[:, E["players_alive"]] == P) and np.all(outs[1][3] == 1) and not outs[1][0].any()


def _npcs_near(d, e, P, reach):
    """Slots of the NPCs in the realm within L-inf `reach` of some player in the realm."""
    ent = d["ent"][e].astype(np.int64)
    pl = np.flatnonzero(ent[F["alive"], :P] != 0)
    out = []
    for s in np.flatnonzero(ent[F["alive"], P:] != 0) + P:
        far = np.maximum(np.abs(ent[F["row"], pl] - ent[F["row"], s]), np.abs(ent[F["col"], pl] - ent[F["col"], s]))
        if len(pl) and far.min() <= reach:
            out.append(int(s))
    return out


def _no_npc_decides(name, blob, post, P, S):
    """Every scenario but A5 (which places its NPCs itself) parks the NPCs more than 10 tiles from
    every player; the ones spawned within 10 tiles of the scenario's band are passive or neutral
    (SPEC §5.7: hostile from 52 tiles off the border), so none attacks unprovoked, and no player
    was hit by an NPC (their ids are negative)."""
    pre = split_state(blob, N, S, P)
    for e in range(N):
        assert not _npcs_near(pre, e, P, 10), f"{name}: env {e} starts with an NPC within 10 tiles of a player"
        if not post["env"][e, E["done"]] and post["env"][e, E["episode"]] == pre["env"][e, E["episode"]]:
            near = _npcs_near(post, e, P, 10)
            assert np.all(post["ent"][e, F["npc_type"], near] < 3), f"{name}: env {e} a hostile NPC spawned near the players"
    assert np.all(post["ent"][:, F["attacker_id"], :P] >= 0), f"{name}: a player was hit by an NPC"


def _buy_outcomes(builder, P=128):
    cfg, blob, acts, witness = builder(P, 256, "C4")
    pre = split_state(blob, N, P + 256, P)
    return witness, [ts.buy_model(pre, e, P, acts[0])[1] for e in range(N)], pre


def test_b1_winner_is_not_the_lowest_slot():
    """B1 shows the Philox order only if it differs from slot order."""
    _, outs, _ = _buy_outcomes(ts.B1)
    for e, out in enumerate(outs):
        order = [b for b, *_ in out]
        assert order != sorted(order) and order[0] != min(order), f"env {e}"
        assert sum(1 for *_, ok in out if ok) == 1


def test_b3_full_reaches_both_outcomes():
    _, outs, _ = _buy_outcomes(ts.B3_full)
    for e, out in enumerate(outs):
        ok = sum(1 for *_, s in out if s)
        assert ok >= 16 and len(out) - ok >= 16, f"env {e}: {ok} of {len(out)} buys succeed"


def test_b3_full_order_matters():
    """The players with room succeed whatever the order, so both outcomes are counted among the
    full buyers alone: at least 16 succeed only because their own listing was bought first, and at
    least 16 whose listing is bought later in Buy order (or not at all) fail."""
    _, outs, pre = _buy_outcomes(ts.B3_full)
    for e, out in enumerate(outs):
        full = {b for b in range(128) if len(ts.inv_of(pre, e, b)) == 12}
        good = sum(1 for b, *_, s in out if s and b in full)
        bad = sum(1 for b, *_, s in out if not s and b in full)
        assert good >= 16 and bad >= 16, f"env {e}: {good} full buyers succeed, {bad} fail"


def test_b4_reaches_both_outcomes():
    witness, outs, _ = _buy_outcomes(ts.B4)
    for e, out in enumerate(outs):
        ok = {b: s for b, *_, s in out}
        yes = sum(1 for a, _ in witness.pairs[e] if ok[a])
        assert yes >= 8 and len(witness.pairs[e]) - yes >= 8, f"env {e}: {yes} of {len(witness.pairs[e])}"


def test_envs_differ_and_actions_are_explicit():
    for name, builder, P, NPC, preset in CASES:
        if P != 128 or preset != "C4":
            continue
        cfg, blob, acts, _ = builder(P, NPC, preset)
        d = split_state(blob, N, P + NPC, P)
        assert not np.array_equal(d["ent"][0, F["col"], :P], d["ent"][1, F["col"], :P]), name
        assert np.array_equal(acts[-1], ts.noop(P, 1)[0]), f"{name}: the last tick is the no-op row"
