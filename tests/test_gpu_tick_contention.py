"""The tick's Buy, Give, Attack and cull ordering on contended states on MI355X, bit-exact against
the CPU oracle (tests/tick_scenarios.py builds the states and their witnesses;
tests/test_tick_scenarios.py shows on the CPU that they reach the contention claimed). Per scenario
and size: a fresh NmmoEngine, set_state, the explicit actions; after every tick the whole state,
rew / term / trunc / mask and the event log equal the oracle's, after the first and the last tick
the flat obs too, the fault word stays 0 (these are legal states: no test expects or raises it), and
the scenario's witness and check_invariants hold on the HIP post-state itself. Every comparison is
bit-exact.

Sizes: everything at C4 128 / 256 (tick_kernel<ALL, 384, 128>), the Attack scenarios at C3 too
(tick_kernel_w8<C3, 384, 128>, the slim entity table), B1 / G1 / A1 / M1 at 100 / 50 (the generic
kernel, S no multiple of 8, a partial wave).

Which scenario and assertion fail when a mechanism of csrc/tick.hip is wrong:
  Rounds (atomicMax keys in two alternating arrays, early retirement, the P + 1 / S + 1 bounds):
    Buy -- B1 (127 buyers of one listing retire in round 1 or 2: "buy: gold" / the single BUY_ITEM),
    B3 and B3_full (a ring: every buy shares a player with two others; a retirement rule too eager
    drops a buy whose room comes from an earlier one: "buy: env e player p inventory"), B4 (gold
    that arrives by an earlier buy: "buy: gold differs"); Give -- G1 (127 gives on one receiver, one
    round each), G2 (a 100-long dependency chain, the gold reaches the last player only if every
    give follows the previous one: "env 0: gold"); Attack -- A1 (127 dependent attacks, 127 rounds,
    the longest a state allows with 128 players), A1_lethal / A6 (a slot killed in an earlier round
    must not act: "attack: ... melee_exp differs"), A2 (44 attacks on one target, the
    lowest pending slot of each round decides the killer: "player_kills differs"). The bound itself:
    get_fault() == 0 with the longest chains.
  Shuffled Buy order (Philox keys four per LDS read, popcount ranks of okm / frm / frow): B1 (the
    winner is the argmin of (key, id), computed in numpy), B2 (12 winners, BUY / EARN pairs in Buy
    order: "buy: events differ"), B5 (rows freed by stacking enter the free ring in Buy order, not
    slot order: "buy: freed rows", which a wrong below(frm) fails; has_room ignoring stacks fails
    B5 and G1). The equal-key path (eq > 1, with its `q < s` tie-break by slot) needs a 32-bit
    Philox collision between two buyers of one tick; no state can be built to reach it, so the
    tie-break stays untested.
  Deferred ammunition and loot (parallel shots of non-victims, thread 0's walk of c.order): A4 --
    last units fired by killers, by non-killers and by victims before they die, loots into full,
    nearly full and stacking inventories ("combat: freed rows": the ring's tail is the serial
    sequence, the shooter's row before its loot's rows; "combat: events": LOOT_ITEM per killer in
    slot order after every attack event); A5 -- NPC drops taken from the ring's head with room for
    one of two, a player killed by an NPC (nothing looted, rows freed in the cull); A2 at C4 --
    30 attackers whose target died before their turn hold equipped ammunition, half of them a last
    unit: a `fired` flag set for a dropped attack shows as "skipped attacker p used ammunition" /
    "a row of skipped attacker p was freed", loot credited to another attacker of the round as
    "LOOT_ITEM not at the killer" / "loot outside the killer"; the victim's own last Arrow is fired
    (env 0) or looted unfired (env 1: its attack is dropped); the gold of A2's and A6's victims
    ("gold differs").
  Packed block scans: ring_ev_append / the Give scan -- G1 (a freed row per stacking gift and up
    to two events per giver in one scan: "give: freed rows", "give: events"); the Move / Sell scan at
    128 | 128 -- M2 ("Move / Sell events": LIST_ITEM placed by its own prefix alone fails the three
    M2 cases), with event_cap 64 and 100 wrapping inside the tick (power-of-two and modulo paths:
    the event log against the oracle's; two events of one scan on one ring row must leave the
    later one, ev_put's c.ev_end); the cull scan at the maximum of all three fields (128 dead
    rows, 128 events, 1,536 item rows) -- M1 ("cull: freed rows", the AGENT_CULLED list,
    item_free_count == 12 P; an event field of 6 bits fails M1 and, with their 64 deaths,
    A1_lethal and A6).
  Position hash and harvest allocation: H1_one_tile (128 players in one bucket chain, only slot 0
    eats and the tile is Scrub afterwards), H1_distinct (128 distinct tiles, the table at its
    fullest, fault word 0),
    H1_professions (0, 1 or 2 rows per player from one prefix sum, the ration before the on-tile
    item: "harvest: inventory").
  Shared scratch: test_back_to_back runs B3, then A1 on one engine; the round keys (c.ft) and the
  flags in c.wtot + 16..31 that Buy, Give and Attack share carry nothing over."""

import numpy as np
import pytest
import torch

from tests import obs_scenarios as sc
from tests import tick_scenarios as ts
from tests.conftest import gpu_available
from tests.test_gpu_parity import _cmp_events, _cmp_state

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

N = ts.N_ENVS
CASES = ts.cases()


def _engine(cfg):
    from nmmo_amd.engine import NmmoEngine

    eng = NmmoEngine(cfg, N, seed=3)
    sc.set_tasks(eng, cfg.PLAYER_N)
    return eng


def _same_obs(eng, orc, where):
    got = eng.obs.cpu().numpy().reshape(orc.obs.shape)
    if not np.array_equal(got.view(np.int32), orc.obs.view(np.int32)):
        bad = np.argwhere(got.view(np.int32) != orc.obs.view(np.int32))[:5]
        raise AssertionError(f"{where}: flat obs differ at (env, agent, entry) {bad.tolist()}")


def _walk(eng, orc, blob, acts, witness, where):
    """set_state on both, then tick by tick: HIP == oracle, fault word 0, witness on the HIP state."""
    P, S = eng.P, eng.S
    eng.set_state(blob)
    orc.set_state(blob)
    torch.cuda.synchronize()
    assert np.array_equal(eng.get_state(), blob), f"{where}: set_state / get_state round trip"
    ticks = acts.shape[0]
    t_now = [0]

    def step(a):
        t = t_now[0]
        orc.step(a)
        eng.step(torch.from_numpy(np.ascontiguousarray(a)).to(eng.device))
        torch.cuda.synchronize()
        at = f"{where} tick {t}"
        assert eng.get_fault() == 0, f"{at}: fault word"
        _cmp_state(eng.get_state(), orc.get_state(), N, S, at, P)
        for name in ("rew", "term", "trunc", "mask"):
            assert np.array_equal(getattr(eng, name).cpu().numpy(), getattr(orc, name)), f"{at}: {name}"
        _cmp_events(eng, orc, N, at)
        if t in (0, ticks - 1):
            _same_obs(eng, orc, at)
        t_now[0] += 1

    ts.run(step, eng.get_state, eng.events, blob, acts, P, S, witness)


@pytest.mark.parametrize("name,builder,P,NPC,preset", CASES, ids=[c[0] for c in CASES])
def test_scenario_on_hip(name, builder, P, NPC, preset):
    cfg, blob, acts, witness = builder(P, NPC, preset)
    eng, orc = _engine(cfg), ts.make_oracle(cfg)
    _walk(eng, orc, blob, acts, witness, name)
    if hasattr(witness, "outputs"):  # the first tick's outputs were compared; the last ones are the auto-reset's
        assert np.all(eng.mask.cpu().numpy() == 1) and not eng.rew.cpu().numpy().any()
    eng.close()


def test_back_to_back():
    """B3, then A1 on one engine: set_state, tick, set_state, tick."""
    cfg, blob_b, acts_b, wit_b = ts.B3()
    _, blob_a, acts_a, wit_a = ts.A1()
    eng, orc = _engine(cfg), ts.make_oracle(cfg)
    _walk(eng, orc, blob_b, acts_b[:1], wit_b, "B3 first")
    _walk(eng, orc, blob_a, acts_a[:1], wit_a, "A1 after B3")
    _walk(eng, orc, blob_b, acts_b[:1], wit_b, "B3 after A1")
    eng.close()
