"""Case builders for the wrapper pass (csrc/wrap.hip, SPEC.md §13) on built event rows.

A scripted rollout never logs two rows of one (event, type, level) tuple for one agent in one
tick, more rows than the kernel has threads, a tuple at a word edge of the `experienced` bitset,
a row that belongs to no agent, or a ring that wraps between two walks. Here such row sets are
built directly and appended to an env's ring with the inject_events test hook (NmmoEngine and
OracleEnvs both have it); the wrapper walks them with the rows of the env's next step.

A case is a Config, a state (a quiet blob from tests/tick_scenarios.py: players on painted Grass,
NPCs parked, so a no-op tick logs next to nothing; or a plain reset) and a schedule of row batches,
one per step. `expectation(case)` drives the schedule through the CPU oracle env -- which only
supplies the tick's own rows, the raw rewards and the flags -- and computes what the wrapper must
hold after every step with the reference's own functions alone (oracle/wrapper.py
count_unique_events over a Python set, process_event_log over the agent's whole log): `Model`.
tests/test_wrapper_cases.py asserts each case's witness on that expectation (CPU),
tests/test_gpu_wrapper_states.py compares the HIP wrapper state with it word for word.

The second half selects tick scenarios (tests/tick_scenarios.py, plus D1 with equipped armor) to
run with the wrapper on against OracleEnvs + OracleWrapper, each with the witnesses it was chosen
for (`oracle_walk` computes them on the oracle side), and builds the saturated obs states with
NPCs of every type for the wrappers' obs edits (`saturated_npcs`, `edited_obs`).

Not a conftest: a plain module the two tests import."""

from __future__ import annotations

import numpy as np

from nmmo_amd import abi
from oracle.oracle import OracleEnvs, join_state, split_state
from oracle.wrapper import EVERY_EVENT_TO_COUNT, count_unique_events, process_event_log
from tests import obs_scenarios as sc
from tests import tick_scenarios as ts
from tests.test_oracle import NOOP

N_ENVS = ts.N_ENVS
E, F, EC, COL = abi.E, abi.F, abi.EventCode, abi.ATTR_TO_COL
CODES = (1, 2, 3, 11, 12, 21, 22, 23, 24, 25, 26, 31, 32, 33, 34, 41, 91)  # SPEC §11's code list, in order
N_TYPES, N_LEVELS = 18, 16
SEED = 17
CLIP, W_EXPLORE = 3, 0.01
AGENT, AGENT_KW = "neurips23_start_kit", dict(explore_bonus_weight=W_EXPLORE)  # the synthetic cases' wrapper
EMPTY = np.zeros((0, abi.EVENT_COLS), np.int32)
assert sorted(v for k, v in vars(EC).items() if k.isupper()) == list(CODES)


def row(ent, code, typ=0, lvl=0, num=0, gold=0, tgt=0, tick=0):
    return [0, ent, tick, code, typ, lvl, num, gold, tgt]


def rows_of(lst):
    return np.array(lst, np.int32).reshape(-1, abi.EVENT_COLS)


def in_range(code, typ, lvl) -> bool:
    return code in CODES and 0 <= typ < N_TYPES and 0 <= lvl < N_LEVELS


def bit_index(code, typ, lvl) -> int:
    """SPEC §13.1: b = (ci * 18 + type) * 16 + level."""
    return (CODES.index(code) * N_TYPES + typ) * N_LEVELS + lvl


def tuple_of_bit(b: int):
    ci, r = divmod(b, N_TYPES * N_LEVELS)
    return (CODES[ci],) + divmod(r, N_LEVELS)


def bitset(tuples) -> np.ndarray:
    """u32 [153] of a set of (event, type, level) tuples; tuples outside §11's ranges have no bit."""
    w = np.zeros(abi.UNIQ_WORDS, np.uint32)
    for t in tuples:
        if in_range(*t):
            b = bit_index(*t)
            w[b // 32] |= np.uint32(1 << (b % 32))
    return w


def countable(rows):
    """The rows whose tuple the wrapper counts at all (SPEC §13.1): in §11's ranges, or of a code
    that counts on every row."""
    keep = [in_range(int(r[3]), int(r[4]), int(r[5])) or int(r[3]) in EVERY_EVENT_TO_COUNT for r in rows]
    return rows[np.array(keep, bool)] if len(rows) else rows


class Model:
    """What the wrapper holds per agent after walking batches of rows: a `set` of tuples and a
    count through count_unique_events, every accumulator through process_event_log over the
    agent's whole log, the return and the start kit's explore bonus in Python floats."""

    def __init__(self, P):
        self.P = P
        self.seen, self.log, self.prev, self.curr, self.cum, self.acc = ({} for _ in range(6))
        for e in range(N_ENVS):
            self.reset_env(e)

    def reset_env(self, e):
        P = self.P
        self.seen[e] = [set() for _ in range(P)]
        self.log[e] = [EMPTY for _ in range(P)]
        self.prev[e], self.curr[e] = np.zeros(P, np.int64), np.zeros(P, np.int64)
        self.cum[e] = [0.0] * P
        self.acc[e] = [None] * P

    def walk(self, e, rows, present, raw, done):
        """One wrapper launch over env e: `rows` are the ring rows between its cursor and the
        event count; present / raw / done [P] are the tick's mask, reward and term | trunc.
        Returns the shaped rewards float32 [P]."""
        rows = rows_of(rows)
        ids = rows[:, COL["ent_id"]]
        out = np.array(raw, np.float32)
        for a in range(1, self.P + 1):
            mine = rows[ids == a]
            if len(mine):
                self.log[e][a - 1] = np.concatenate([self.log[e][a - 1], mine])
                self.acc[e][a - 1] = None
            n = count_unique_events(countable(mine), self.seen[e][a - 1])
            if not present[a - 1]:
                continue
            self.prev[e][a - 1] = self.curr[e][a - 1]
            self.curr[e][a - 1] += n
            if not done[a - 1]:
                self.cum[e][a - 1] += float(raw[a - 1])
            r, explore = float(raw[a - 1]), 0
            if W_EXPLORE > 0 and n > 0:  # neurips23_start_kit/reward_wrapper.py:63-82, heal weight 0
                explore = min(CLIP, n) * W_EXPLORE
            r += 0 + explore
            out[a - 1] = np.float32(r)
        return out

    def accumulators(self, e, a):
        if self.acc[e][a - 1] is None:
            log = self.log[e][a - 1]
            ach, perf = process_event_log(log)
            hit = log[:, COL["event"]] == EC.SCORE_HIT
            self.acc[e][a - 1] = dict(
                performed=sum(1 << b for b, k in enumerate(abi.PERFORMED_KEYS) if perf["event/" + k]),
                max_dist=ach["achieved/max_progress_to_center"], earned_gold=ach["achieved/earned_gold"],
                max_damage=ach["achieved/max_damage"],
                max_item_level=[ach.get(f"achieved/max_{c}_level", -1) for c in abi.ITEM_CATEGORIES],
                agent_kills=ach["achieved/agent_kill_count"], npc_kills=ach["achieved/npc_kill_count"],
                dmg_inflicted=int(log[hit, COL["damage"]].sum()))  # SPEC §13.2's decision
        return self.acc[e][a - 1]

    def state(self):
        """NmmoWrapState records [N_ENVS, P] (abi.wrap_state_dtype) under the start kit wrapper."""
        st = np.zeros((N_ENVS, self.P), abi.wrap_state_dtype())
        st["hp"] = 100
        for e in range(N_ENVS):
            st["cum_reward"][e] = self.cum[e]
            st["prev_count"][e], st["curr_count"][e] = self.prev[e], self.curr[e]
            st["prev_price"][e] = NOOP[10]
            for a in range(1, self.P + 1):
                for k, v in self.accumulators(e, a).items():
                    st[k][e, a - 1] = v
        return st

    def bitsets(self):
        return np.stack([np.stack([bitset(s) for s in self.seen[e]]) for e in range(N_ENVS)])


def expected_info(st, e, a, tick, log, cum, eval_mode, term):
    """SPEC §13.5: the info dict of agent a's final step from the post-step state and its log."""
    ent = lambda f: int(st["ent"][e, F[f], a - 1])  # noqa: E731
    t = st["tstate"][e][a - 1]
    maxp, sig = float(t["max_progress"]), int(t["signals"])
    stats = {"cod/attacked": float(term and ent("damage") > 0), "cod/starved": float(term and ent("food") == 0),
             "cod/dehydrated": float(term and ent("water") == 0),
             "task/completed": float(int(t["completed_tick"]) != 0), "task/pcnt_2_reward_signal": float(sig >= 2),
             "task/pcnt_0p2_max_progress": float(maxp >= 0.2),
             "achieved/max_combat_level": max(ent("melee_level"), ent("range_level"), ent("mage_level")),
             "achieved/max_harvest_skill_ammo": max(ent("prospecting_level"), ent("carving_level"), ent("alchemy_level")),
             "achieved/max_harvest_skill_consum": max(ent("fishing_level"), ent("herbalism_level"))}
    ach, perf = process_event_log(log)
    for k, v in list(ach.items()) + list(perf.items()):
        stats[k] = float(v)
    return {"stats": stats, "length": int(tick), "return": maxp if eval_mode else cum, "curriculum": {"task": (maxp, sig)}}


class Case:
    def __init__(self, name, cfg, blob, batches, witness, end=None, only=None, tasks=True, eval_mode=False):
        self.name, self.cfg, self.blob, self.batches, self.witness = name, cfg, blob, batches, witness
        self.end, self.only, self.tasks, self.eval_mode = end or {}, only or {}, tasks, eval_mode
        self.P = cfg.PLAYER_N
        self.S = cfg.PLAYER_N + (cfg.NPC_N if "NPC" in cfg.systems else 0)

    def prepare(self, handle):
        """The case's start state on an OracleEnvs or an NmmoEngine (whose wrapper is already on)."""
        if self.tasks:
            sc.set_tasks(handle, self.P)
        if self.blob is None:
            handle.reset()
        else:
            handle.set_state(self.blob)

    def actions(self):
        return np.tile(np.array(NOOP, np.int32), (N_ENVS, self.P, 1))


class Snap:
    """The expectation after one step of a case."""


def expectation(case):
    """[Snap] per step of the case, from the CPU oracle env and `Model`. Cached on the case."""
    if getattr(case, "_snaps", None) is not None:
        return case._snaps
    orc = OracleEnvs(case.cfg, N_ENVS, seed=SEED)
    case.prepare(orc)
    P, S, cap = case.P, case.S, case.cfg.event_cap
    m = Model(P)
    acts = case.actions()
    count = [int(c) for c in split_state(orc.get_state(), N_ENVS, S, P)["env"][:, E["event_count"]]]
    pending = [EMPTY] * N_ENVS
    dropped, snaps = 0, []
    for t, batch in enumerate(case.batches):
        for e, rows in sorted(batch.items()):
            orc.inject_events(e, rows)
            pending[e] = np.concatenate([pending[e], rows_of(rows)])
        if t in case.end:
            orc.end_episodes(np.array(case.end[t], np.uint8))
        envs = list(case.only.get(t, range(N_ENVS)))
        if t in case.only:
            for e in envs:
                orc.step_range(e, e + 1, acts)
        else:
            orc.step(acts)
        st = split_state(orc.get_state(), N_ENVS, S, P)
        s = Snap()
        s.raw = orc.rew.copy()
        s.envs, s.rew, s.infos, s.walked, s.grown = envs, orc.rew.copy(), [{} for _ in range(N_ENVS)], [EMPTY] * N_ENVS, [0] * N_ENVS
        s.term, s.trunc, s.mask = orc.term.copy(), orc.trunc.copy(), orc.mask.copy()
        for e in envs:
            tick, new = int(st["env"][e, E["tick"]]), int(st["env"][e, E["event_count"]])
            if tick == 0:  # the env was reset in this step: the wrapper starts over, rewards untouched
                m.reset_env(e)
                count[e], pending[e] = new, EMPTY
                continue
            grown = new - count[e]
            count[e] = new
            ev = orc.events(e)
            k = min(grown, cap)
            walked = ev[len(ev) - k:] if k else EMPTY
            skip = grown - k  # rows the ring overwrote before the walk
            dropped += skip
            inj = pending[e][skip:]  # the rows injected since the env's last step come first, as given
            assert np.array_equal(walked[:len(inj)], inj), f"{case.name} step {t} env {e}: injected rows read back"
            pending[e] = EMPTY
            done = (orc.term[e] | orc.trunc[e]) != 0
            s.rew[e] = m.walk(e, walked, orc.mask[e], orc.rew[e], done)
            s.walked[e], s.grown[e] = walked, grown
            for a in range(1, P + 1):
                if orc.mask[e, a - 1] and done[a - 1]:
                    s.infos[e][a] = expected_info(st, e, a, tick, m.log[e][a - 1], m.cum[e][a - 1], case.eval_mode,
                                                  bool(orc.term[e, a - 1]))
        s.state, s.uniq, s.dropped, s.count = m.state(), m.bitsets(), dropped, list(count)
        s.events = [orc.events(e) for e in range(N_ENVS)]
        s.gain = [m.curr[e] - m.prev[e] for e in range(N_ENVS)]
        snaps.append(s)
    case._snaps = snaps
    return snaps


# ---------------------------------------------------------------- states
def quiet(P, N, tick=None, **kw):
    """(cfg, blob): tick_scenarios' base state with the players along one painted Grass row per env."""
    cfg, d = ts.base(P, N, "C4", **kw)
    for e in range(N_ENVS):
        ts.snake(d, e, P)
        d["ent"][e, F["exploration"], :P] = 64  # no tile is a new record: no GO_FARTHEST of the tick's own
    if tick is not None:
        d["env"][:, E["tick"]] = tick
    cfg, blob, _, _ = ts.finish(cfg, d, P, P + N, None, None)
    return cfg, blob


def _payload(k):
    return dict(num=1 + (7 * k) % 50, gold=k % 13, tgt=(k % 9 + 1) * (1 if k % 2 else -1))


# ---------------------------------------------------------------- the cases
EDGE_BITS = (31, 32, 63, 64, 4895)


def W1(P=128, N=256):
    """Edges: for slot 0, slot P - 1 and a few between, every code with (type, level) in {0, 17} x
    {0, 15} and the tuples of bits 31, 32, 63, 64 and 4895; the same rows again in a second step
    (only PLAYER_KILL / EARN_GOLD rows count then)."""
    cfg, blob = quiet(P, N)
    batch = {}
    for e in range(N_ENVS):
        agents = (1, 2, P // 2, P - 1, P) if e == 0 else (1, 3, P // 2 + 1, P)
        lst, k = [], 0
        for a in agents:
            tuples = [(c, ty, lv) for c in CODES for ty in (0, 17) for lv in (0, 15)] + [tuple_of_bit(b) for b in EDGE_BITS]
            for c, ty, lv in tuples:
                lst.append(row(a, c, ty, lv, **_payload(k)))
                k += 1
        batch[e] = rows_of(lst if e == 0 else lst[::-1])

    def witness(snaps):
        for e in range(N_ENVS):
            uq = snaps[0].uniq[e]
            for sl in (0, P - 1):
                assert uq[sl, 0] >> 31 & 1 and uq[sl, 1] & 1 and uq[sl, 1] >> 31 & 1 and uq[sl, 2] & 1, "bits 31, 32, 63, 64"
                assert uq[sl, 152] >> 31 & 1 and uq[sl, 0] & 1, "bits 0 and 4895"
                n_pk = int(np.sum((batch[e][:, 1] == sl + 1) & np.isin(batch[e][:, 3], list(EVERY_EVENT_TO_COUNT))))
                assert snaps[1].gain[e][sl] == n_pk > 0, "the second walk counts only PLAYER_KILL / EARN_GOLD rows"
            assert np.array_equal(snaps[0].uniq[e] & snaps[1].uniq[e], snaps[0].uniq[e])
    return Case(f"W1-{P}", cfg, blob, [batch, batch], witness)


def W2(P=128, N=256):
    """Duplicates: 3 copies of one tuple per agent, a whole pass of the agents apart, and for one
    agent 300 copies each of a SCORE_HIT, a PLAYER_KILL and an EARN_GOLD tuple: one row wins per
    tuple, PLAYER_KILL / EARN_GOLD count every time."""
    cfg, blob = quiet(P, N)
    batch, star = {}, {0: 5, 1: P}
    for e in range(N_ENVS):
        lst = [row(a, EC.HARVEST_ITEM, 2 + (a + e) % 16, (a + 3 * e) % 16, 1) for _ in range(3) for a in range(1, P + 1)]
        x = star[e]
        for i in range(300):
            lst.append(row(x, EC.SCORE_HIT, 1 + e, 0, num=1 + (i * 37) % 97))
            lst.append(row(x, EC.PLAYER_KILL, 0, 3, tgt=7 if i % 3 else -4))
            lst.append(row(x, EC.EARN_GOLD, 0, 0, gold=1 + i % 5))
        batch[e] = rows_of(lst)

    def witness(snaps):
        for e in range(N_ENVS):
            w, x = snaps[0].walked[e], star[e]
            assert len(w) > 256 and int(np.sum(w[:, 1] == x)) >= 257
            own = w[w[:, 1] == x]
            per_code = {c: count_unique_events(own[own[:, 3] == c], set()) for c in (EC.SCORE_HIT, EC.PLAYER_KILL, EC.EARN_GOLD)}
            assert per_code == {EC.SCORE_HIT: 1, EC.PLAYER_KILL: 300, EC.EARN_GOLD: 300}
            others = np.delete(np.arange(P), x - 1)
            assert snaps[0].gain[e][x - 1] == 602 > CLIP and np.all(snaps[0].gain[e][others] >= 1)
            st = snaps[0].state[e, x - 1]
            assert st["max_damage"] == 97 and st["agent_kills"] == 200 and st["npc_kills"] == 100
            assert st["earned_gold"] == 900 and st["dmg_inflicted"] == int(own[own[:, 3] == EC.SCORE_HIT, 6].sum())
            raw = float(snaps[0].raw[e, x - 1])  # 602 new counts earn the clipped bonus, 3 x the weight
            assert snaps[0].rew[e, x - 1] == np.float32(raw + CLIP * W_EXPLORE) != np.float32(raw + 602 * W_EXPLORE)
    return Case(f"W2-{P}", cfg, blob, [batch], witness)


def W3(P=128, N=256):
    """Skipped rows: valid rows interleaved with rows of ent_id 0, P + 1, -5 and 2^31 - 1 (they
    belong to nobody) and rows of valid agents with type -1 / 18 / 31, level -1 / 16 or code 99 (no
    bit, no unique count; the accumulators read them as process_event_log does)."""
    cfg, blob = quiet(P, N)
    batch = {}
    for e in range(N_ENVS):
        good = (1, 2 + e, P)
        lst = []
        for i in range(40):
            a = good[i % 3]
            lst.append(row(a, CODES[i % 17], (i * 5 + e) % 18, (i * 3) % 16, **_payload(i)))
            for bad in (0, P + 1, -5, 2**31 - 1):  # in-range tuples: a missing id check would set their bits
                lst.append(row(bad, CODES[(i + 1) % 17], (i + e) % 18, i % 16, **_payload(i + 1)))
            lst += [row(a, EC.EAT_FOOD, -1, 0), row(a, EC.HARVEST_ITEM, 18, 2, 1), row(a, EC.EQUIP_ITEM, 31, 1),
                    row(a, EC.LOOT_ITEM, 3, 16, 1), row(a, EC.SCORE_HIT, 1, -1, num=9 + i), row(a, EC.GO_FARTHEST, 0, 16, num=12 + i),
                    row(a, 99, 1, 1, num=1000, gold=1000, tgt=3), row(a, EC.PLAYER_KILL, 18, 3, tgt=-2),
                    row(a, EC.EARN_GOLD, 0, 16, gold=5)]
        batch[e] = rows_of(lst)

    def witness(snaps):
        for e in range(N_ENVS):
            good = (1, 2 + e, P)
            idle = [a for a in range(1, P + 1) if a not in good]
            s = snaps[0]
            tick_only = rows_of([r for r in s.walked[e] if r[1] in idle])
            m = Model(P)
            m.walk(e, tick_only, s.mask[e], np.zeros(P, np.float32), np.zeros(P, bool))
            for a in idle:  # out-of-range ids change nothing anywhere
                assert np.array_equal(s.uniq[e, a - 1], bitset(m.seen[e][a - 1]))
            for a in good:
                st = s.state[e, a - 1]
                assert st["max_item_level"][0] == 16 and st["max_damage"] >= 9 and st["max_dist"] >= 12
                assert st["npc_kills"] > 0 and st["earned_gold"] >= 5
                own = s.walked[e][s.walked[e][:, 1] == a]
                assert s.gain[e][a - 1] < count_unique_events(own, set()), "the reference's set would count the odd tuples"
    return Case(f"W3-{P}", cfg, blob, [batch], witness)


def W4(cap, P=128, N=256):
    """The ring between walks: a filler batch, then cap - 5 rows that straddle the ring's end
    (nothing dropped), then cap + 37 rows (exactly the overwritten ones are dropped, the last cap
    are walked)."""
    cfg, blob = quiet(P, N, event_cap=cap)

    def rows(n, base, e):
        return rows_of([row((7 * (i + base) + e) % P + 1, CODES[(i + base) % 17], (i + base) % 18, (i + base + e) % 16, **_payload(i + base))
                        for i in range(n)])
    sizes = (cap // 2 + 7, cap - 5, cap + 37)
    batches = [{e: rows(n, 1000 * t, e) for e in range(N_ENVS)} for t, n in enumerate(sizes)]

    def witness(snaps):
        for e in range(N_ENVS):
            c0, c1, c2 = (s.count[e] for s in snaps)
            assert c1 - c0 <= cap and c0 % cap > c1 % cap, "the second batch straddles the ring's end"
            assert snaps[1].dropped == 0
            assert c2 - c1 > cap and len(snaps[2].walked[e]) == cap
            assert np.array_equal(snaps[2].walked[e], snaps[2].events[e])
        assert snaps[2].dropped == sum(snaps[2].grown[e] - cap for e in range(N_ENVS)) > 0
    return Case(f"W4-cap{cap}", cfg, blob, batches, witness)


def W5(eval_mode=False, P=128, N=256):
    """Finals: a history for every agent over two steps, a few more rows in the third, which
    truncates everyone (E_TICK = HORIZON - 3 in the blob): P records per env in one launch."""
    cfg, blob = quiet(P, N, tick=ts.config(P, N).HORIZON - 3)
    item = (2, 5, 8, 13, 16)  # one category per agent: the others stay absent (level -1)
    batches = []
    for t in range(3):
        batch = {}
        for e in range(N_ENVS):
            lst = []
            for a in range(1, P + 1):
                k = a + e
                if t == 0:
                    lst += [row(a, EC.GO_FARTHEST, num=1 + k % 20), row(a, EC.SCORE_HIT, 1 + k % 3, 0, num=1 + (3 * k) % 40),
                            row(a, EC.HARVEST_ITEM, item[k % 5], 1 + k % 10, 1), row(a, EC.EARN_GOLD, gold=1 + k % 7)]
                    if k % 2 == 0:
                        lst.append(row(a, EC.EQUIP_ITEM, 2 + k % 14, 1 + k % 5))
                elif t == 1:
                    lst += [row(a, EC.GO_FARTHEST, num=1 + (5 * k) % 23), row(a, EC.SCORE_HIT, 1 + k % 3, 0, num=1 + (11 * k) % 60),
                            row(a, EC.PLAYER_KILL, 0, 1 + k % 4, tgt=-3 if k % 3 == 0 else k % P + 1), row(a, EC.EAT_FOOD)]
                    if k % 4 == 0:
                        lst += [row(a, EC.LOOT_ITEM, 6, 1 + k % 6, 1, tgt=2), row(a, EC.LIST_ITEM, 6, 1, 1, gold=9)]
                    if k % 5 == 1:
                        lst.append(row(a, EC.BUY_ITEM, 16, 2 + k % 3, 1, gold=4))
                else:
                    lst += [row(a, EC.EARN_GOLD, gold=2), row(a, EC.CONSUME_ITEM, 16 + k % 2, 1, 1)]
                    if k % 6 == 0:
                        lst.append(row(a, EC.DRINK_WATER))
            batch[e] = rows_of(lst)
        batches.append(batch)

    def witness(snaps):
        assert not snaps[0].infos[0] and not snaps[1].infos[1]
        for e in range(N_ENVS):
            assert np.all(snaps[2].trunc[e] == 1) and not snaps[2].term[e].any()
            inf = snaps[2].infos[e]
            assert sorted(inf) == list(range(1, P + 1)), "a record for every agent in one launch"
            absent = [sum(1 for a in inf if f"achieved/max_{c}_level" not in inf[a]["stats"]) for c in abi.ITEM_CATEGORIES]
            assert all(0 < n < P for n in absent), absent
            assert len({inf[a]["stats"]["achieved/unique_events"] for a in inf}) > 2
            assert any(inf[a]["return"] != 0 for a in inf)
    return Case(f"W5-eval{int(eval_mode)}", cfg, blob, batches, witness, eval_mode=eval_mode)


def W6():
    """The scalar bitset clear: PLAYER_N = 3 (3 * 153 words are no multiple of 4, env 1's bitsets
    start 12 bytes past a 16-byte boundary). Rows into both envs, then env 0's episode is ended:
    its wrapper state and bitsets return to their initial values, env 1's are untouched."""
    from nmmo_amd.config import Config

    cfg = Config.preset("C2", MAP_N=4, PLAYER_N=3, early_stop_agent_num=0)
    P = 3
    batch = {e: rows_of([row(1 + (i + e) % P, CODES[i % 17], (i * 5) % 18, (i + e) % 16, **_payload(i)) for i in range(60)])
             for e in range(N_ENVS)}

    def witness(snaps):
        assert (P * abi.UNIQ_WORDS) % 4 != 0 and (P * abi.UNIQ_WORDS * 4) % 16 != 0
        a, b = snaps
        assert a.uniq[0].any() and a.uniq[1].any() and not np.array_equal(a.uniq[0], a.uniq[1])
        assert not b.uniq[0].any() and np.array_equal(b.state[0], Model(P).state()[0]), "env 0 is back to initial"
        assert np.array_equal(b.uniq[1] & a.uniq[1], a.uniq[1]) and np.all(b.state["curr_count"][1] >= a.state["curr_count"][1])
        assert np.all(a.state["curr_count"] > 0)
    return Case("W6", cfg, None, [batch, {}], witness, end={1: [1, 0]}, tasks=False)


def WP(P=128, N=256):
    """Partial lists: rows into both envs, then a step of env 1 only: env 0's wrapper state, bitsets
    and cursor stay, and its rows are walked by its own later step, exactly once."""
    cfg, blob = quiet(P, N)
    batch = {e: rows_of([row((3 * i + e) % P + 1, CODES[i % 17], (i + e) % 18, i % 16, **_payload(i)) for i in range(300)])
             for e in range(N_ENVS)}

    def witness(snaps):
        a, b, c = snaps
        init = Model(P).state()[0]
        assert np.array_equal(a.state[0], init) and not a.uniq[0].any() and a.uniq[1].any()
        assert len(b.walked[0]) >= 300 and np.array_equal(b.walked[0][:300], batch[0])
        assert np.all(b.gain[0] > 0) and np.array_equal(b.uniq[1] & a.uniq[1], a.uniq[1])
        assert c.grown[0] < 300 and len(c.walked[0]) == c.grown[0] and np.array_equal(c.state["curr_count"][0] - c.gain[0], b.state["curr_count"][0])
    return Case(f"WP-{P}", cfg, blob, [batch, {}, {}], witness, only={0: [1]})


def cases():
    """[(id, builder, args)]: W1-W3 at 128 / 256 and at 100 / 50, the rest at 128 / 256 (W6 at 3 / 0)."""
    out = [(f"{f.__name__}-{P}", f, (P, N)) for f in (W1, W2, W3) for P, N in ((128, 256), (100, 50))]
    out += [("W4-cap64", W4, (64,)), ("W4-cap100", W4, (100,)), ("W5-eval0", W5, (False,)), ("W5-eval1", W5, (True,)),
            ("W6", W6, ()), ("WP-128", WP, ())]
    return out


_built: dict = {}


def build(cid):
    """The case of id `cid`, built once per process (the expectation is cached on it)."""
    if cid not in _built:
        _, f, args = next(c for c in cases() if c[0] == cid)
        _built[cid] = f(*args)
    return _built[cid]


# ---------------------------------------------------------------- contended tick scenarios, wrapper on
YAOFENG_KW = dict(hp_bonus_weight=0.03, exp_bonus_weight=0.002, defense_bonus_weight=0.04, attack_bonus_weight=0.001,
                  gold_bonus_weight=0.001, custom_bonus_scale=0.5)  # every weight non-zero
KIT_KW = dict(heal_bonus_weight=0.03, explore_bonus_weight=0.01)
KIT, YAO, TAK = "neurips23_start_kit", "yaofeng", "takeru"


def D1(P=128, N=256, preset="C4"):
    """Equipped armor and tools (none of tick_scenarios' states has any): level-1 Hat / Top / Bottom
    and a tool in every combination over the players, gold that differs per player, two no-op ticks.
    YAOFENG's defense term is non-zero and differs between agents."""
    cfg, d = ts.base(P, N, preset)
    for e in range(N_ENVS):
        ts.snake(d, e, P)
        d["ent"][e, F["gold"], :P] = [(3 * p + e) % 40 for p in range(P)]
        for p in range(P):
            k = (p + e) % 16
            for bit, typ in enumerate((2, 3, 4, 8 + p % 5)):
                if k >> bit & 1:
                    ts._one_item(d, e, p, typ, 1, eq=1)
            if p % 3 == 0:
                ts._one_item(d, e, p, 16, 2)  # an unequipped ration: no defense
    return ts.finish(cfg, d, P, P + N, ts.noop(P), None)
# (id, tick_scenarios builder, P, N, preset, agent, kwargs, witnesses the oracle side must reach)
SCENARIOS = [
    ("M1-yaofeng-128", ts.M1, 128, 256, "C4", YAO, YAOFENG_KW, ("finals_all", "cod")),
    ("M1-yaofeng-100", ts.M1, 100, 50, "C4", YAO, YAOFENG_KW, ("finals_all", "cod")),
    ("M2_cap64-kit", ts.M2_cap64, 128, 256, "C4", KIT, KIT_KW, ("dropped", "price")),
    ("M2_cap100-kit", ts.M2_cap100, 128, 256, "C4", KIT, KIT_KW, ("dropped", "price")),
    ("A4-yaofeng", ts.A4, 128, 256, "C4", YAO, YAOFENG_KW, ("agent_kill", "loot", "hits")),
    ("A4-kit", ts.A4, 128, 256, "C4", KIT, KIT_KW, ("gain_above_clip", "agent_kill")),
    ("D1-yaofeng", D1, 128, 256, "C4", YAO, YAOFENG_KW, ("defense",)),
    ("A5-yaofeng", ts.A5, 128, 256, "C4", YAO, YAOFENG_KW, ("npc_kill", "loot")),
    ("A5-kit", ts.A5, 128, 256, "C4", KIT, KIT_KW, ("gain_above_clip", "npc_kill")),
    ("A1-C3-yaofeng", ts.A1, 128, 256, "C3", YAO, YAOFENG_KW, ("no_items", "hits")),
    ("A3-kit", ts.A3, 128, 256, "C4", KIT, KIT_KW, ("level_up", "hits")),  # H1_professions levels nobody up
    ("B2-kit", ts.B2, 128, 256, "C4", KIT, KIT_KW, ("earn_gold_repeats",)),
    ("G1-takeru", ts.G1, 128, 256, "C4", TAK, dict(explore_bonus_weight=0.01), ("give_edit",)),
    ("H1_professions-kit", ts.H1_professions, 128, 256, "C4", KIT, KIT_KW, ("harvest", "gain_is_clip")),
]


def oracle_state(ow):
    """(fields, bitsets) of everything an OracleWrapper holds that NmmoWrapState restates: the counts,
    the return, prev_price, YAOFENG's previous values, the `experienced` set as a bitset, and the
    accumulators as process_event_log gives them over the agent's log so far."""
    P = ow.P
    st = np.zeros((N_ENVS, P), abi.wrap_state_dtype())
    uq = np.zeros((N_ENVS, P, abi.UNIQ_WORDS), np.uint32)
    for e in range(N_ENVS):
        m = Model(P)
        ids = ow.log[e][:, COL["ent_id"]]
        for a in ow.ids:
            u, d = ow.uniq[e][a], ow.data[e][a]
            m.log[e][a - 1] = ow.log[e][ids == a]
            r = st[e, a - 1]
            r["cum_reward"], r["prev_count"], r["curr_count"] = ow.cum[e][a], u["prev_count"], u["curr_count"]
            r["prev_price"], r["hp"], r["exp"], r["gold"] = ow.hist[e][a]["prev_price"], d["hp"], d["exp"], d["gold"]
            r["dmg_inflicted_prev"] = d["damage_inflicted"]
            for k, v in m.accumulators(e, a).items():
                r[k] = v
            uq[e, a - 1] = bitset(u["experienced"])
    return st, uq


def _defense(st, e, a):
    D = 0
    for w0, _ in st["items"][e][a - 1]:
        t, lvl, eq = int(w0) & 31, (int(w0) >> 5) & 15, (int(w0) >> 9) & 1
        if t and eq:
            D += 3 * lvl if 2 <= t <= 4 else 2 * lvl if 8 <= t <= 12 else 0
    return D


def oracle_walk(builder, P, N, preset, agent, kw, on_tick=None, orc=None, blob_acts=None):
    """A tick scenario through the oracle env and a fresh OracleWrapper, tick by tick. Returns
    the set of witnesses reached; on_tick(t, ticks, orc, ow, acts, dropped) runs after every tick."""
    from oracle.wrapper import OracleWrapper

    cfg, blob, acts, _ = builder(P, N, preset) if blob_acts is None else blob_acts
    orc = ts.make_oracle(cfg) if orc is None else orc
    orc.set_state(blob)
    ow = OracleWrapper(orc, agent, **kw)
    S, cap = orc.S, cfg.event_cap
    lay = ow.lay
    reached, dropped = set(), 0
    if "Item" not in cfg.systems:
        reached.add("no_items")
    count = split_state(blob, N_ENVS, S, P)["env"][:, E["event_count"]].astype(np.int64)
    for t in range(acts.shape[0]):
        orc.step(acts[t])
        raw_obs = None if orc.obs is None else orc.obs.copy()
        ow.after_step(acts[t])
        st = ow._state()
        for e in range(N_ENVS):
            if st["env"][e][E["tick"]] == 0:
                count[e] = st["env"][e][E["event_count"]]
                continue
            new = int(st["env"][e][E["event_count"]])
            if new - count[e] > cap:
                dropped += int(new - count[e] - cap)
                reached.add("dropped")
            count[e] = new
            rows = orc.events(e)
            rows = rows[rows[:, COL["tick"]] == st["env"][e][E["tick"]]]
            kills = rows[rows[:, 3] == EC.PLAYER_KILL]
            reached |= {"npc_kill"} if np.any(kills[:, 8] < 0) else set()
            reached |= {"agent_kill"} if np.any(kills[:, 8] > 0) else set()
            for name, code in (("loot", EC.LOOT_ITEM), ("harvest", EC.HARVEST_ITEM), ("level_up", EC.LEVEL_UP), ("hits", EC.SCORE_HIT)):
                if np.any(rows[:, 3] == code):
                    reached.add(name)
            gold = rows[rows[:, 3] == EC.EARN_GOLD]
            if len(gold) and max(np.unique(gold[:, [1, 4, 5]], axis=0, return_counts=True)[1]) > 1:
                reached.add("earn_gold_repeats")
            present = [a for a in ow.ids if orc.mask[e, a - 1]]
            gains = [ow.uniq[e][a]["curr_count"] - ow.uniq[e][a]["prev_count"] for a in present]
            clip = ow.w.get("clip_unique_event", 3)
            reached |= {"gain_above_clip"} if any(g > clip for g in gains) else set()
            reached |= {"gain_is_clip"} if any(g == clip for g in gains) else set()
            if len(ow.infos[e]) == P:
                reached.add("finals_all")
            if any(i["stats"]["cod/starved"] == 1.0 for i in ow.infos[e].values()):
                reached.add("cod")
            if "Item" in cfg.systems and any(_defense(st, e, a) > 0 for a in present if not (orc.term[e, a - 1] or orc.trunc[e, a - 1])):
                reached.add("defense")
            if np.any(acts[t][e, :, 10] != 0):
                reached.add("price")
            if raw_obs is not None:
                for seg in ("Give.Target", "Give.InventoryItem", "GiveGold.Target"):
                    s = lay["ActionTargets." + seg]
                    if np.any(raw_obs[e][:, s.offset:s.offset + s.shape[0]] != orc.obs[e][:, s.offset:s.offset + s.shape[0]]):
                        reached.add("give_edit")
        if on_tick is not None:
            on_tick(t, acts.shape[0], orc, ow, acts[t], dropped)
    return reached


# ---------------------------------------------------------------- obs edits at saturation
def saturated_npcs(P=128, N=256):
    """obs_scenarios' saturated pair (100 shown entities, a full market; the same with a group out of
    the realm) with the first three NPCs beside the crowd made of npc_type 1, 2 and 3 (another order
    in env 1), so a full window holds passive, neutral and hostile rows."""
    out = []
    for blob in sc.saturated_pair(P, N, sc.GROUP_OUT):
        d = split_state(blob, N_ENVS, P + N, P)
        for e in range(N_ENVS):
            live = [s for s in range(P, P + N) if d["ent"][e, F["alive"], s]][:3]
            d["ent"][e, F["npc_type"], live] = (1, 2, 3) if e == 0 else (3, 1, 2)
        out.append(join_state(d))
    return out


def edited_obs(orc, agent, kw, prev_price=None):
    """(raw, edited) flat obs [N_ENVS, P, elems] of the oracle's current state: the oracle's rows,
    and the same after OracleWrapper._observation (prev_price [N_ENVS, P]: the start kit's history)."""
    from oracle.wrapper import OracleWrapper

    raw = np.stack([orc.flat_obs(e) for e in range(N_ENVS)])
    keep = orc.obs
    orc.obs = raw.copy()
    ow = OracleWrapper(orc, agent, **kw)
    st = ow._state()
    for e in range(N_ENVS):
        if prev_price is not None:
            for a in ow.ids:
                ow.hist[e][a]["prev_price"] = int(prev_price[e, a - 1])
        ow._observation(e, st, np.ones(orc.P, np.uint8))
    edited, orc.obs = orc.obs, keep
    return raw, edited


def obs_edit_witness(raw, edited, lay):
    """Some agent's window holds 100 entity rows with NPCs of npc_type 1, 2 and 3 among them; the
    dangerous-NPC edit clears at least one Attack.Target bit and keeps at least one."""
    en, at = lay["Entity"], lay["ActionTargets.Attack.Target"]
    full = cleared = kept = 0
    for e in range(N_ENVS):
        for p in range(raw.shape[1]):
            rows = raw[e, p, en.offset:en.offset + 3100].reshape(100, 31)
            if np.all(rows[:, 0] != 0) and {1, 2, 3} <= set(rows[:, 1].astype(int).tolist()):
                full += 1
            a0 = raw[e, p, at.offset:at.offset + 100]
            a1 = edited[e, p, at.offset:at.offset + 100]
            cleared += int(np.sum((a0 != 0) & (a1 == 0) & (rows[:, 1] > 1)))
            kept += int(np.sum((a1 != 0) & (rows[:, 0] != 0)))
            assert not np.any((a1 != 0) & (rows[:, 1] > 1)) and not np.any((a0 == 0) & (a1 != 0))
    assert full > 0 and cleared > 0 and kept > 0, (full, cleared, kept)
    return full, cleared, kept
