"""Scenario builders for the tick's Buy, Give, Attack and cull ordering on contended states.

csrc/tick.hip resolves nmmo's one-entity-at-a-time order in parallel (rounds of atomicMax keys for
Buy, Give / GiveGold and Attack, a Philox-shuffled Buy order ranked by popcounts, packed block scans,
a position hash for first-on-tile harvests). Scripted rollouts meet that machinery only by accident,
so the states that load it are built here: each scenario is a function of (P, N, preset) returning
`(cfg, blob, actions, witness)` -- a Config, a valid state blob of N_ENVS = 2 envs that differ (other
slots, other gold, mirrored order), explicit int32 actions [ticks][2][P][12], and a witness
`(pre, post, events) -> None` that asserts the scenario's stated outcome on the state after the
first tick (`pre`, `post`: split_state dicts, `events`: one event array per env). Witnesses are
computed from the pre-state, the actions, SPEC.md constants and Philox alone: `Model` restates
SPEC §9's receive rules, `buy_model` / `give_model` / `attack_model` the serial Buy (shuffled),
Give (slot) and Attack (slot) orders, `combat_model` the attacks with equipment, ammunition, loot
and NPCs; nothing here reads a result except to compare.
tests/test_tick_scenarios.py runs them on the CPU oracle (with the reach conditions: both outcomes
of an order-dependent buy occur), tests/test_gpu_tick_contention.py on the HIP tick.

Action heads (tick.hip's decode): 0 Attack.Style, 1 Attack.Target, 2 Buy.MarketItem, 3 Destroy,
4 Give item, 5 Give target, 6 GiveGold price, 7 GiveGold target, 8 Move, 9 Sell item, 10 Sell
price, 11 Use. Target heads index the actor's shown window (first 100 entities in ascending
datastore row within L-inf <= 7), so 128 players on one tile can name only the first 100 of them.

Not a conftest: a plain module the two tests import."""

from __future__ import annotations

import numpy as np

from nmmo_amd import abi
from oracle.oracle import join_state, split_state
from tests import obs_scenarios as sc
from tests.test_gpu_heads import philox_np
from tests.test_oracle import NOOP

N_ENVS = sc.N_ENVS
E, F, EV, C = abi.E, abi.F, abi.EventCode, abi.ATTR_TO_COL
INV = abi.INV_SLOTS
GRASS, SCRUB, FOILAGE, ORE, FISH = 2, 3, 4, 7, 15  # common.h Material
THRESH = (0, 90, 250, 500, 900, 1500, 2400, 3700, 5500, 8000)  # SPEC §1 exp -> level
P_BUY_ORDER = 7
STYLE_EXP = ("melee_exp", "range_exp", "mage_exp")
STYLE_LVL = ("melee_level", "range_level", "mage_level")
SKILL_LVL = STYLE_LVL + ("fishing_level", "herbalism_level", "prospecting_level", "carving_level", "alchemy_level")
ROW0 = 20  # the scenarios' band: rows 18..32, at most 16 tiles from the border (spawned NPCs: passive)

H_ASTYLE, H_ATGT, H_BUY, H_DESTROY, H_GIVE, H_GIVET, H_GGP, H_GGT, H_MOVE, H_SELL, H_SELLP, H_USE = range(12)


def config(P=128, N=256, preset="C4", **kw):
    from nmmo_amd.config import Config

    return Config.preset(preset, MAP_N=4, early_stop_agent_num=0, PLAYER_N=P, NPC_N=N, **kw)


def level_of(exp: int) -> int:
    return sum(1 for t in THRESH if t <= exp)


# ---------------------------------------------------------------- item words (SPEC §9)
def w0(typ, lvl=1, eq=0, price=0, ltick=0):
    return typ | lvl << 5 | eq << 9 | price << 10 | ltick << 17


def it_type(w): return int(w[0]) & 31
def it_level(w): return int(w[0]) >> 5 & 15
def it_eq(w): return int(w[0]) >> 9 & 1
def it_price(w): return int(w[0]) >> 10 & 127
def it_qty(w): return int(w[1]) & 0xFFFF
def it_row(w): return int(w[1]) >> 16


def inv_of(d, e, p):
    return [[int(a), int(b)] for a, b in d["items"][e, p] if int(a) & 31]


# ---------------------------------------------------------------- the base state and its edits
_base_cache: dict = {}


def base(P, N, preset, **kw):
    """(cfg, split reset state) with every NPC parked on the far border row, players past their
    spawn immunity, at food = water = 50 (no regeneration, no starvation), no items, no gold."""
    key = (P, N, preset, tuple(sorted(kw.items())))
    if key not in _base_cache:
        cfg = config(P, N, preset, **kw)
        _base_cache[key] = (cfg, sc.reset_blob(cfg))
    cfg, blob = _base_cache[key]
    S = P + N
    d = split_state(blob, N_ENVS, S, P)
    for e in range(N_ENVS):
        ent = d["ent"][e]
        ent[F["time_alive"], :P] = 30
        ent[F["food"], :P] = ent[F["water"], :P] = 50
        npcs = [s for s in range(P, S) if ent[F["alive"], s]]
        for j, s in enumerate(npcs):  # bottom border row (Grass by construction), > 100 tiles away
            ent[F["row"], s], ent[F["col"], s] = 143, 16 + j % 128
    return cfg, d


def paint(d, e, r0, r1, c0=16, c1=143, m=GRASS):
    """Rows r0..r1, cols c0..c1 (inside the playable area) become material m."""
    assert 16 <= r0 <= r1 <= 143 and 16 <= c0 <= c1 <= 143
    d["mat"][e, r0:r1 + 1, c0:c1 + 1] = m


def snake(d, e, P, row=ROW0, slots=None):
    """Players along one painted row, consecutive slots adjacent; env 1 runs the other way on another row."""
    row += 5 * e
    paint(d, e, row - 1, row + 1)
    for i, s in enumerate(range(P) if slots is None else slots):
        d["ent"][e, F["row"], s] = row
        d["ent"][e, F["col"], s] = 16 + i if e == 0 else 143 - i
    return row


def one_tile(d, e, slots, r, c):
    paint(d, e, r - 1, r + 1, c - 1, c + 1)
    for s in slots:
        d["ent"][e, F["row"], s], d["ent"][e, F["col"], s] = r, c


def shown(d, e, p, S):
    """Slots of p's shown window: in the realm, L-inf <= 7, ascending datastore row, first 100 (SPEC §8)."""
    ent = d["ent"][e].astype(np.int64)
    sl = np.flatnonzero(ent[F["alive"]] != 0)
    sl = sl[np.argsort(ent[F["ds_row"], sl], kind="stable")]
    near = np.maximum(np.abs(ent[F["row"], sl] - ent[F["row"], p]), np.abs(ent[F["col"], sl] - ent[F["col"], p])) <= 7
    return sl[near][:100].tolist()


def target_index(d, e, p, t, S):
    vis = shown(d, e, p, S)
    assert t in vis, f"env {e}: slot {t} is not in slot {p}'s shown window"
    return vis.index(t)


def listing_index(d, e, P, row):
    rows = sc.priced_rows(d, e, P)[0][:abi.MARKET_ROWS].tolist()
    assert row in rows
    return rows.index(row)


def noop(P, ticks=2):
    return np.tile(np.array(NOOP, np.int32), (ticks, N_ENVS, P, 1))


def check_blob(d, P, S):
    """The builder rules: a valid state (check_invariants), gold far below 32,767."""
    check_invariants(d, P, S)
    assert int(d["ent"][:, F["gold"], :P].astype(np.int64).sum(axis=1).max()) < 32767
    assert not np.array_equal(d["ent"][0], d["ent"][1]), "the two envs must differ"


def finish(cfg, d, P, S, acts, witness, items=True):
    if items and "Item" in cfg.systems:
        for e in range(N_ENVS):
            sc._finish_items(d, e, P)
    check_blob(d, P, S)
    return cfg, join_state(d), acts, witness


def check_invariants(d, P, S, events=None):
    """Item rows in inventories unique and in 1..12P; inventory rows + free-ring rows = exactly 1..12P;
    inventories compact and ascending by row; item_level = the equipped levels; 0 <= gold,
    0 <= health <= 100; players_alive matches the table; with `events` (the retained log rows per
    env) the event ids are consecutive and end at event_count, from 1 unless the ring has wrapped."""
    IC = INV * P
    for e in range(d["env"].shape[0]):
        env, ent = d["env"][e], d["ent"][e]
        rows = []
        for p in range(P):
            it = d["items"][e, p]
            n = sc._ninv(it)
            r = (it[:n, 1] >> 16).astype(np.int64)
            assert np.all(np.diff(r) > 0), f"env {e} player {p}: inventory not ascending by row"
            rows += r.tolist()
            eq = ((it[:n, 0] >> 9) & 1) != 0
            assert ent[F["item_level"], p] == int(((it[:n, 0] >> 5) & 15)[eq].sum()), f"env {e} player {p}: item_level"
        head, cnt = int(env[E["item_free_head"]]), int(env[E["item_free_count"]])
        free = [int(d["iring"][e, (head + i) % IC]) for i in range(cnt)]
        assert sorted(rows + free) == list(range(1, IC + 1)), f"env {e}: item rows are not exactly 1..{IC}"
        assert np.all(ent[F["gold"], :P] >= 0), f"env {e}: negative gold"
        assert np.all((ent[F["health"]] >= 0) & (ent[F["health"]] <= 100)), f"env {e}: health out of range"
        assert env[E["players_alive"]] == int((ent[F["alive"], :P] != 0).sum()), f"env {e}: players_alive"
        if events is not None:
            ids, n = events[e][:, C["id"]].astype(np.int64), int(env[E["event_count"]])
            assert len(ids) <= n and (len(ids) > 0) == (n > 0), f"env {e}: {len(ids)} event rows of {n} logged"
            want = np.arange(n - len(ids) + 1, n + 1)  # from 1 when every row was kept
            assert np.array_equal(ids, want), f"env {e}: event ids are not consecutive up to {n}"


# ---------------------------------------------------------------- SPEC restatements
class Model:
    """Inventories, gold and the item free ring's tail of one env, with SPEC §9's receive rules."""

    def __init__(self, pre, e, P):
        self.e, self.P = e, P
        self.inv = [inv_of(pre, e, p) for p in range(P)]
        self.gold = pre["ent"][e, F["gold"], :P].astype(np.int64).copy()
        self.freed: list = []    # rows appended to the free ring, in order
        self.events: list = []   # (ent_id, event, type, level, number, gold, target_ent)

    def stack_slot(self, p, w):
        if not 13 <= it_type(w) <= 15:
            return -1
        return next((k for k, x in enumerate(self.inv[p]) if it_type(x) == it_type(w) and it_level(x) == it_level(w)), -1)

    def has_room(self, p, w):
        return self.stack_slot(p, w) >= 0 or len(self.inv[p]) < INV

    def receive(self, p, w):
        """An existing item arrives: ammunition merges (its row is freed), else a free slot, else destroyed."""
        k = self.stack_slot(p, w)
        if k >= 0:
            self.inv[p][k][1] += it_qty(w)
            self.freed.append(it_row(w))
        elif len(self.inv[p]) >= INV:
            self.freed.append(it_row(w))
        else:
            self.inv[p].append([int(w[0]), int(w[1])])
            self.inv[p].sort(key=it_row)

    def find(self, p, row):
        return next((k for k, x in enumerate(self.inv[p]) if it_row(x) == row), -1)

    def log(self, p, code, typ=0, lvl=0, num=0, gold=0, tgt=0):
        self.events.append((p + 1, code, typ, lvl, num, gold, tgt))

    # ---- comparisons with a post-state
    def assert_items(self, post, what):
        e = self.e
        for p in range(self.P):
            assert inv_of(post, e, p) == self.inv[p], f"{what}: env {e} player {p} inventory"
        got = post["ent"][e, F["gold"], :self.P].astype(np.int64)
        assert np.array_equal(got, self.gold), f"{what}: env {e} gold differs at {np.flatnonzero(got != self.gold)[:8].tolist()}"

    def assert_freed(self, pre, post, what):
        """The rows this model freed are the free ring's new tail, in this order."""
        e, IC = self.e, INV * self.P
        tail = int(pre["env"][e, E["item_free_head"]]) + int(pre["env"][e, E["item_free_count"]])
        got = [int(post["iring"][e, (tail + i) % IC]) for i in range(len(self.freed))]
        assert got == self.freed, f"{what}: env {e} freed rows {got[:12]} != {self.freed[:12]} (first 12)"
        assert int(post["env"][e, E["item_free_count"]]) == int(pre["env"][e, E["item_free_count"]]) + len(self.freed), \
            f"{what}: env {e} item_free_count"

    def assert_events(self, pre, events, codes, what):
        assert_events(pre, events, self.e, codes, self.events, what)


def assert_events(pre, events, e, codes, want, what):
    """The first tick's events with a code in `codes`, in log order, equal `want`."""
    ev = events[e]
    ev = ev[(ev[:, C["tick"]] == pre["env"][e, E["tick"]] + 1) & np.isin(ev[:, C["event"]], codes)]
    got = [tuple(int(x) for x in r[[1, 3, 4, 5, 6, 7, 8]]) for r in ev]
    want = [tuple(int(x) for x in w) for w in want]
    if got != want:
        k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"{what}: env {e} events differ ({len(got)} rows, want {len(want)}) at {k}: "
                             f"got {got[k] if k < len(got) else None} want {want[k] if k < len(want) else None}")


def acts_at_turn(pre, e, p):
    """In the realm with health > 0 after the update phase (SPEC §5.2: regeneration, starvation)."""
    return bool(pre["ent"][e, F["alive"], p]) and updated_health(pre, e, p) > 0


def updated_health(pre, e, p):
    ent = pre["ent"][e]
    h = int(ent[F["health"], p])
    if p >= pre["items"].shape[1]:
        return min(100, h + 1)
    food, water = int(ent[F["food"], p]), int(ent[F["water"], p])
    if food > 50 and water > 50:
        h = min(100, h + 10)
    hurt = 5 if ent[F["resilient"], p] else 10
    for v in (food, water):
        if v == 0:
            h = max(0, h - hurt)
    return h


def buy_keys(pre, e, slots):
    """draw(tick, BUY_ORDER, id, 0)[0] of the players in `slots` (SPEC §2, §9)."""
    env = pre["env"][e]
    lo, hi = int(env[E["seed_lo"]]) & 0xFFFFFFFF, int(env[E["seed_hi"]]) & 0xFFFFFFFF
    return philox_np(int(env[E["tick"]]), P_BUY_ORDER, np.asarray(slots, np.uint64) + np.uint64(1), 0, lo, hi)


def buy_order(pre, e, slots):
    """`slots` in Buy order: ascending (Philox key, id)."""
    keys = buy_keys(pre, e, slots)
    return [s for _, s in sorted(zip(keys.tolist(), slots))]


def buy_model(pre, e, P, acts):
    """SPEC §9 Buy, serially in Buy order -> (model, [(buyer, owner, row, price, succeeded)] in Buy order)."""
    m = Model(pre, e, P)
    rows, _, _ = sc.priced_rows(pre, e, P)
    rows = rows[:abi.MARKET_ROWS].tolist()
    want = {p: rows[acts[e, p, H_BUY]] for p in range(P)
            if pre["ent"][e, F["alive"], p] and 0 <= acts[e, p, H_BUY] < len(rows)}
    out = []
    for b in buy_order(pre, e, sorted(want)):
        row = want[b]
        owner = next((q for q in range(P) if m.find(q, row) >= 0), -1)
        ok = False
        price = 0
        if acts_at_turn(pre, e, b) and owner >= 0 and owner != b:
            w = m.inv[owner][m.find(owner, row)]
            price = it_price(w)
            if price and m.gold[b] >= price and m.has_room(b, w):
                ok = True
                m.gold[b] -= price
                m.gold[owner] += price
                m.log(b, EV.BUY_ITEM, it_type(w), it_level(w), it_qty(w), price)
                m.log(owner, EV.EARN_GOLD, gold=price)
                m.inv[owner].pop(m.find(owner, row))
                m.receive(b, [w[0] & 0x1FF, w[1]])
        out.append((b, owner, row, price, ok))
    return m, out


def give_model(pre, e, P, S, acts):
    """SPEC §9 Give and GiveGold, serially in slot order (the item first)."""
    m = Model(pre, e, P)
    ent = pre["ent"][e]

    def ok_target(p, t):
        return (0 <= t < P and t != p and acts_at_turn(pre, e, t)
                and ent[F["row"], t] == ent[F["row"], p] and ent[F["col"], t] == ent[F["col"], p])

    dec = {}
    for p in range(P):  # decode against the pre-state (SPEC §5.0)
        if not ent[F["alive"], p]:
            continue
        vis, a = shown(pre, e, p, S), acts[e, p]
        inv0 = inv_of(pre, e, p)
        grow = it_row(inv0[a[H_GIVE]]) if 0 <= a[H_GIVE] < len(inv0) and 0 <= a[H_GIVET] < len(vis) else -1
        gt = vis[a[H_GIVET]] if grow >= 0 else -1
        ggt, amt = (vis[a[H_GGT]], int(a[H_GGP]) + 1) if 0 <= a[H_GGT] < len(vis) and 0 <= a[H_GGP] < 99 else (-1, 0)
        dec[p] = (grow, gt, ggt, amt)
    for p in sorted(dec):
        if not acts_at_turn(pre, e, p):
            continue
        grow, gt, ggt, amt = dec[p]
        if grow >= 0 and ok_target(p, gt):
            k = m.find(p, grow)
            if k >= 0 and not it_eq(m.inv[p][k]) and not it_price(m.inv[p][k]) and m.has_room(gt, m.inv[p][k]):
                w = m.inv[p].pop(k)
                m.log(p, EV.GIVE_ITEM, it_type(w), it_level(w), it_qty(w), 0, int(ent[F["id"], gt]))
                m.receive(gt, w)
        if ggt >= 0 and ok_target(p, ggt) and amt <= m.gold[p]:
            m.gold[p] -= amt
            m.gold[ggt] += amt
            m.log(p, EV.GIVE_GOLD, gold=amt, tgt=int(ent[F["id"], ggt]))
    return m


def damage(st, style, x, t):
    """SPEC §1: int(max(mult * offense - defense, 0.25 * offense)), no equipment, on the skills as
    they stand at the attack (an earlier attack of the target's own has moved its exp)."""
    offense = 10 + 5 * int(st[STYLE_LVL[style]][x])
    defense = 5 * max(int(st[k][t]) for k in SKILL_LVL)
    exps = [int(st[k][t]) for k in STYLE_EXP]
    mult4 = 4
    if max(exps) != min(exps):
        dom = exps.index(max(exps))
        if style == (2, 0, 1)[dom]:  # Mage beats Melee, Melee beats Range, Range beats Mage
            mult4 = 6
    return max(mult4 * offense - 4 * defense, offense) // 4


def attack_model(pre, e, P, S, acts, exchange):
    """SPEC §5.3 Attack among players without equipment, serially in slot order. Returns the
    expected fields per player and the attack events."""
    ent = pre["ent"][e].astype(np.int64)
    tick1 = int(pre["env"][e, E["tick"]]) + 1
    st = {k: ent[F[k], :P].copy() for k in ("health", "gold", "player_kills", "latest_combat_tick") + STYLE_EXP + SKILL_LVL}
    st["health"] = np.array([updated_health(pre, e, p) for p in range(P)])
    st["damage"] = np.zeros(P, np.int64)
    st["attacker_id"] = np.zeros(P, np.int64)
    events, executed, skipped = [], [], []
    for x in range(P):
        if not ent[F["alive"], x]:
            continue
        vis, a = shown(pre, e, x, S), acts[e, x]
        if not (0 <= a[H_ASTYLE] < 3 and 0 <= a[H_ATGT] < len(vis)):
            continue
        t, sty = vis[a[H_ATGT]], int(a[H_ASTYLE])
        assert t < P, "attack_model covers players only"
        reach = max(abs(ent[F["row"], x] - ent[F["row"], t]), abs(ent[F["col"], x] - ent[F["col"], t])) <= 3
        if not (st["health"][x] > 0 and st["health"][t] > 0 and t != x and ent[F["time_alive"], t] + 1 >= 20 and reach):
            skipped.append(x)
            continue
        executed.append(x)
        dmg = damage(st, sty, x, t)
        st[STYLE_EXP[sty]][x] += 6
        events.append((x + 1, EV.SCORE_HIT, sty + 1, 0, dmg, 0, 0))
        nl = level_of(int(st[STYLE_EXP[sty]][x]))
        if nl > st[STYLE_LVL[sty]][x]:
            st[STYLE_LVL[sty]][x] = nl
            events.append((x + 1, EV.LEVEL_UP, sty + 1, nl, 0, 0, 0))
        st["attacker_id"][t], st["damage"][t] = x + 1, dmg
        st["health"][t] = max(0, st["health"][t] - dmg)
        if st["health"][t] == 0:
            st["player_kills"][x] += 1
            events.append((x + 1, EV.PLAYER_KILL, 0, max(int(ent[F[k], t]) for k in STYLE_LVL), 0, 0, t + 1))
            if exchange:
                st["gold"][x] += st["gold"][t]
                st["gold"][t] = 0
        st["latest_combat_tick"][x] = st["latest_combat_tick"][t] = tick1
    return st, events, executed, skipped


def _eq_offense(inv, style):
    return sum(5 + 5 * it_level(w) for w in inv if it_eq(w) and it_type(w) in (5 + style, 13 + style))


def _eq_defense(inv):
    return sum(3 * it_level(w) if 2 <= it_type(w) <= 4 else 2 * it_level(w) if 8 <= it_type(w) <= 12 else 0
               for w in inv if it_eq(w))


def combat_model(pre, e, P, S, acts, npc_attacks=()):
    """SPEC §5.3 and §9 with every system on: the attacks of the players (from `acts`) and of the NPCs
    in `npc_attacks` [(slot, target slot)] serially in slot order, with equipment, ammunition, loot
    and the cull's destruction of unlooted items. Returns (fields [S], Model, attack events + loot
    events, executed, skipped)."""
    ent = pre["ent"][e].astype(np.int64)
    IC = INV * P
    tick1 = int(pre["env"][e, E["tick"]]) + 1
    m = Model(pre, e, P)
    keys = ("health", "gold", "player_kills", "latest_combat_tick") + STYLE_EXP + SKILL_LVL
    st = {k: ent[F[k]].copy() for k in keys}
    st["health"] = np.array([updated_health(pre, e, s) if ent[F["alive"], s] else 0 for s in range(S)])
    st["damage"], st["attacker_id"] = np.zeros(S, np.int64), np.zeros(S, np.int64)
    attacks = []
    for x in range(P):
        vis, a = shown(pre, e, x, S), acts[e, x]
        if ent[F["alive"], x] and 0 <= a[H_ASTYLE] < 3 and 0 <= a[H_ATGT] < len(vis):
            attacks.append((x, int(a[H_ASTYLE]), vis[a[H_ATGT]]))
    attacks += [(x, int(ent[F["style"], x]), t) for x, t in npc_attacks]
    events, loots, executed, skipped, by_npc = [], [], [], [], set()
    head, taken = int(pre["env"][e, E["item_free_head"]]), 0
    for x, sty, t in sorted(attacks):
        reach = max(abs(ent[F["row"], x] - ent[F["row"], t]), abs(ent[F["col"], x] - ent[F["col"], t])) <= 3
        immune = x < P and t < P and ent[F["time_alive"], t] + 1 < 20
        if not (st["health"][x] > 0 and st["health"][t] > 0 and t != x and not immune and not (x >= P and t >= P) and reach):
            skipped.append(x)
            continue
        executed.append(x)
        offense = 10 + 5 * int(st[STYLE_LVL[sty]][x]) + (_eq_offense(m.inv[x], sty) if x < P else int(ent[F["equip_offense"], x]))
        defense = 5 * max(int(st[k][t]) for k in (SKILL_LVL if t < P else STYLE_LVL))
        defense += _eq_defense(m.inv[t]) if t < P else int(ent[F["equip_defense"], t])
        exps = [int(st[k][t]) for k in STYLE_EXP]
        mult4 = 6 if max(exps) != min(exps) and sty == (2, 0, 1)[exps.index(max(exps))] else 4
        dmg = max(mult4 * offense - 4 * defense, offense) // 4
        if x < P:
            st[STYLE_EXP[sty]][x] += 6
            events.append((x + 1, EV.SCORE_HIT, sty + 1, 0, dmg, 0, 0))
            nl = level_of(int(st[STYLE_EXP[sty]][x]))
            if nl > st[STYLE_LVL[sty]][x]:
                st[STYLE_LVL[sty]][x] = nl
                events.append((x + 1, EV.LEVEL_UP, sty + 1, nl, 0, 0, 0))
            k = next((k for k, w in enumerate(m.inv[x]) if it_eq(w) and it_type(w) == 13 + sty), -1)
            if k >= 0:  # one unit of the equipped ammunition of this style; the last one frees the row
                m.inv[x][k][1] -= 1
                if it_qty(m.inv[x][k]) == 0:
                    m.freed.append(it_row(m.inv[x].pop(k)))
        st["attacker_id"][t], st["damage"][t] = ent[F["id"], x], dmg
        st["health"][t] = max(0, st["health"][t] - dmg)
        if st["health"][t] == 0:
            st["player_kills"][x] += 1
            if x >= P:
                by_npc.add(t)
            else:
                events.append((x + 1, EV.PLAYER_KILL, 0, max(int(ent[F[k], t]) for k in STYLE_LVL), 0, 0, int(ent[F["id"], t])))
                m.gold[x] += st["gold"][t] if t >= P else m.gold[t]
                if t < P:
                    m.gold[t] = 0
                    for w in m.inv[t]:  # inventory (= row) order, receive rules
                        loots.append((x + 1, EV.LOOT_ITEM, it_type(w), it_level(w), it_qty(w), 0, t + 1))
                        m.receive(x, [w[0] & 0x1FF, w[1]])
                    m.inv[t] = []
                else:  # the NPC's armor piece, then its tool, new items of the NPC's level
                    lvl = max(1, int(ent[F["npc_level"], t]))
                    for typ in (2 + int(ent[F["drop_armor"], t]), 8 + int(ent[F["drop_tool"], t])):
                        loots.append((x + 1, EV.LOOT_ITEM, typ, lvl, 1, 0, int(ent[F["id"], t])))
                        if len(m.inv[x]) < INV:
                            row = int(pre["iring"][e, (head + taken) % IC])
                            taken += 1
                            m.inv[x].append([w0(typ, lvl), 1 | row << 16])
                            m.inv[x].sort(key=it_row)
        st["latest_combat_tick"][x] = st["latest_combat_tick"][t] = tick1
    for p in range(P):  # the cull: what nobody looted is destroyed, in (slot, inventory) order
        if ent[F["alive"], p] and st["health"][p] == 0:
            m.freed += [it_row(w) for w in m.inv[p]]
            m.inv[p] = []
    st["gold"][:P] = m.gold
    m.taken = taken
    return st, m, events + loots, executed, skipped


def assert_combat(pre, post, events, e, P, S, acts, npc_attacks, what):
    st, m, evs, executed, skipped = combat_model(pre, e, P, S, acts, npc_attacks)
    ent = post["ent"][e].astype(np.int64)
    for k, v in st.items():
        got = ent[F[k], :P]
        assert np.array_equal(got, v[:P]), f"{what}: env {e} {k} differs at slots {np.flatnonzero(got != v[:P])[:8].tolist()}"
    was = pre["ent"][e, F["alive"], :P] != 0
    dead = (st["health"][:P] == 0) & was
    assert np.array_equal(ent[F["alive"], :P] != 0, was & ~dead), f"{what}: env {e} culled"
    assert_events(pre, events, e, (EV.SCORE_HIT, EV.LEVEL_UP, EV.PLAYER_KILL, EV.LOOT_ITEM), evs, what)
    assert_events(pre, events, e, (EV.AGENT_CULLED,), [(int(p) + 1, EV.AGENT_CULLED, 0, 0, 0, 0, 0) for p in np.flatnonzero(dead)], what)
    m.assert_items(post, what)
    IC = INV * P  # rows taken from the ring's head (NPC drops), rows appended to its tail
    tail = int(pre["env"][e, E["item_free_head"]]) + int(pre["env"][e, E["item_free_count"]])
    got = [int(post["iring"][e, (tail + i) % IC]) for i in range(len(m.freed))]
    assert got == m.freed, f"{what}: env {e} freed rows {got[:16]} != {m.freed[:16]} (first 16)"
    assert post["env"][e, E["item_free_head"]] == (int(pre["env"][e, E["item_free_head"]]) + m.taken) % IC
    assert post["env"][e, E["item_free_count"]] == pre["env"][e, E["item_free_count"]] - m.taken + len(m.freed)
    return st, m, evs, executed, skipped


def assert_attack(pre, post, events, e, P, S, acts, exchange, what):
    st, evs, executed, skipped = attack_model(pre, e, P, S, acts, exchange)
    ent = post["ent"][e].astype(np.int64)
    for k, v in st.items():
        got = ent[F[k], :P]
        assert np.array_equal(got, v), f"{what}: env {e} {k} differs at slots {np.flatnonzero(got != v)[:8].tolist()}"
    dead = st["health"] == 0
    assert np.array_equal(ent[F["alive"], :P] == 0, dead | (pre["ent"][e, F["alive"], :P] == 0)), f"{what}: env {e} culled"
    assert_events(pre, events, e, (EV.SCORE_HIT, EV.LEVEL_UP, EV.PLAYER_KILL), evs, what)
    culled = [(int(p) + 1, EV.AGENT_CULLED, 0, 0, 0, 0, 0) for p in np.flatnonzero(dead & (pre["ent"][e, F["alive"], :P] != 0))]
    assert_events(pre, events, e, (EV.AGENT_CULLED,), culled, what)
    return st, evs, executed, skipped


# ---------------------------------------------------------------- Buy scenarios
def _one_item(d, e, p, typ, lvl=1, qty=1, **kw):
    n = sc._ninv(d["items"][e, p])
    d["items"][e, p, n] = [w0(typ, lvl, **kw), qty]


def _fill(d, e, p, n, avoid=(13, 14, 15)):
    """Top p's inventory up to n unequipped, unlisted items of non-ammunition types."""
    types = [t for t in (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 16, 17) if t not in avoid]
    k = sc._ninv(d["items"][e, p])
    while k < n:
        d["items"][e, p, k] = [w0(types[(p + k) % len(types)], 1 + (p + 2 * k) % 9), 1]
        k += 1


def _buy_actions(d, P, want, ticks=2):
    """want[e][buyer] = (owner, inventory slot of the listing at build time) -> Buy.MarketItem indices."""
    acts = noop(P, ticks)
    for e in range(N_ENVS):
        for b, (o, k) in want[e].items():
            acts[0, e, b, H_BUY] = listing_index(d, e, P, it_row(d["items"][e, o, k]))
    return acts


def _buy_witness(P, acts, extra):
    def witness(pre, post, events):
        for e in range(N_ENVS):
            m, out = buy_model(pre, e, P, acts[0])
            m.assert_items(post, "buy")
            m.assert_freed(pre, post, "buy")
            m.assert_events(pre, events, (EV.BUY_ITEM, EV.EARN_GOLD), "buy")
            assert int(post["ent"][e, F["gold"], :P].astype(np.int64).sum()) == int(pre["ent"][e, F["gold"], :P].astype(np.int64).sum()), \
                f"env {e}: gold is not conserved"
            extra(pre, post, events, e, m, out)
    return witness


def _listed_slot(d, e, p):
    return next(k for k in range(INV) if it_price(d["items"][e, p, k]))


def B1(P=128, N=256, preset="C4"):
    """One listing, P - 1 buyers: exactly one BUY_ITEM / EARN_GOLD pair, the buyer is the argmin of
    (Philox key, id) over the buyers, gold is conserved, every other inventory untouched."""
    cfg, d = base(P, N, preset)
    S, want = P + N, [{}, {}]
    seller = (0, P - 1)
    for e in range(N_ENVS):
        snake(d, e, P)
        _one_item(d, e, seller[e], 5, 3, price=10 + e, ltick=sc.TICK - 1)
        for p in range(P):
            d["ent"][e, F["gold"], p] = 20 + p + 7 * e
            if p != seller[e]:
                _fill(d, e, p, (p + e) % 12)  # room everywhere, other inventories to leave alone
                want[e][p] = (seller[e], 0)
    for e in range(N_ENVS):
        sc._finish_items(d, e, P)
    acts = _buy_actions(d, P, want)

    def extra(pre, post, events, e, m, out):
        buyers = [p for p in range(P) if p != seller[e]]
        keys = buy_keys(pre, e, buyers).tolist()
        winner = min(zip(keys, buyers))[1]
        ev = events[e]
        buys = ev[ev[:, C["event"]] == EV.BUY_ITEM]
        earns = ev[ev[:, C["event"]] == EV.EARN_GOLD]
        assert len(buys) == 1 and len(earns) == 1, f"env {e}: {len(buys)} BUY_ITEM, {len(earns)} EARN_GOLD"
        assert buys[0, C["ent_id"]] == winner + 1 and earns[0, C["ent_id"]] == seller[e] + 1, f"env {e}: buyer"
        for p in buyers:
            if p != winner:
                assert inv_of(post, e, p) == inv_of(pre, e, p), f"env {e}: player {p}'s inventory changed"
        assert [b for b, *_, ok in out if ok] == [winner]
    return finish(cfg, d, P, S, acts, _buy_witness(P, acts, extra), items=False)


def B2(P=128, N=256, preset="C4"):
    """One seller with 12 listings, P - 1 buyers spread over them: per listing the earliest buyer in
    Buy order wins; the BUY / EARN pairs appear in Buy order."""
    cfg, d = base(P, N, preset)
    S, want = P + N, [{}, {}]
    seller = (3, P - 5)
    for e in range(N_ENVS):
        snake(d, e, P)
        for k in range(INV):
            _one_item(d, e, seller[e], 2 + k, 1 + k % 9, price=1 + k + e, ltick=sc.TICK - 1 - k % 3)
        for p in range(P):
            d["ent"][e, F["gold"], p] = 60 + p + e
            if p != seller[e]:
                want[e][p] = (seller[e], (5 * p + e) % INV)
    for e in range(N_ENVS):
        sc._finish_items(d, e, P)
    acts = _buy_actions(d, P, want)

    def extra(pre, post, events, e, m, out):
        order = buy_order(pre, e, sorted(want[e]))
        first = {}
        for b in order:
            first.setdefault(want[e][b][1], b)
        assert len(first) == INV
        winners = [b for b in order if first[want[e][b][1]] == b]
        assert [b for b, *_, ok in out if ok] == winners, f"env {e}: winners"
        ev = events[e]
        got = ev[ev[:, C["event"]] == EV.BUY_ITEM][:, C["ent_id"]].tolist()
        assert got == [b + 1 for b in winners], f"env {e}: BUY_ITEM order"
    return finish(cfg, d, P, S, acts, _buy_witness(P, acts, extra), items=False)


def B3(P=128, N=256, preset="C4", full=False):
    """Ring of buys: player i lists one item and buys player (i + 1) mod P's. With room everywhere
    all P buys succeed, events in Buy order. `full`: inventories hold 12 items (one listed) except
    every fourth player's 11: a full buyer succeeds iff its own listing was bought earlier in Buy
    order (a ring of full inventories alone admits no buy at all, so some players have room)."""
    cfg, d = base(P, N, preset)
    S, want = P + N, [{}, {}]
    for e in range(N_ENVS):
        snake(d, e, P)
        for p in range(P):
            d["ent"][e, F["gold"], p] = 40 + (5 * p + 11 * e) % 50
            if full:
                _fill(d, e, p, 10 if (p + e) % 4 == 0 else 11)
            _one_item(d, e, p, 2 + (p + e) % 11, 1 + p % 9, price=1 + (3 * p + e) % 30, ltick=sc.TICK - 1)
            want[e][p] = ((p + 1) % P if e == 0 else (p - 1) % P, None)
    for e in range(N_ENVS):
        sc._finish_items(d, e, P)
    acts = noop(P)
    for e in range(N_ENVS):
        for b, (o, _) in want[e].items():
            acts[0, e, b, H_BUY] = listing_index(d, e, P, it_row(d["items"][e, o, _listed_slot(d, e, o)]))

    def extra(pre, post, events, e, m, out):
        ok = {b: s for b, *_, s in out}
        if not full:
            assert all(ok.values()) and len(ok) == P, f"env {e}: not every buy of the ring succeeded"
            return
        pos = {b: i for i, (b, *_) in enumerate(out)}
        for b in range(P):
            prev = next(q for q in range(P) if want[e][q][0] == b)  # the buyer of b's listing
            room0 = len(inv_of(pre, e, b)) < INV
            assert ok[b] == (room0 or (ok[prev] and pos[prev] < pos[b])), f"env {e}: buyer {b}"
    return finish(cfg, d, P, S, acts, _buy_witness(P, acts, extra), items=False)


def B3_full(P=128, N=256, preset="C4"):
    return B3(P, N, preset, full=True)


B3_full.__doc__ = B3.__doc__


def B4(P=128, N=256, preset="C4"):
    """Gold from a sale: P / 2 pairs (a, b). b lists at price p and, with ample gold, buys a's listing
    at price q; a holds p - q and buys b's listing: it succeeds iff b's buy precedes a's."""
    cfg, d = base(P, N, preset)
    S, want, pairs = P + N, [{}, {}], [[], []]
    for e in range(N_ENVS):
        snake(d, e, P)
        for i in range(P // 2):
            a, b = (2 * i, 2 * i + 1) if e == 0 else (2 * i + 1, 2 * i)
            p_, q = 30 + (i + e) % 40, 5 + i % 20
            _one_item(d, e, a, 2 + i % 11, 1 + i % 9, price=q, ltick=sc.TICK - 1)
            _one_item(d, e, b, 16 + i % 2, 1 + i % 9, price=p_, ltick=sc.TICK - 1)
            d["ent"][e, F["gold"], a], d["ent"][e, F["gold"], b] = p_ - q, 200 + i + e
            want[e][a], want[e][b] = (b, 0), (a, 0)
            pairs[e].append((a, b))
    for e in range(N_ENVS):
        sc._finish_items(d, e, P)
    acts = _buy_actions(d, P, want)

    def extra(pre, post, events, e, m, out):
        pos = {b: i for i, (b, *_) in enumerate(out)}
        ok = {b: s for b, *_, s in out}
        for a, b in pairs[e]:
            assert ok[b], f"env {e}: b = {b}"
            assert ok[a] == (pos[b] < pos[a]), f"env {e}: a = {a}"
    w = _buy_witness(P, acts, extra)
    w.pairs = pairs  # per env [(a, b)]: the CPU test counts both outcomes of a's buy
    return finish(cfg, d, P, S, acts, w, items=False)


def B5(P=128, N=256, preset="C4"):
    """Stacking frees rows: buyers with 12 items including an ammunition stack buy a listed stack of
    the same type and level (room by stacking: quantities add, the incoming row is freed, appended
    to the free ring in Buy order); full buyers without the stack, after the same listings, fail."""
    cfg, d = base(P, N, preset)
    S, want, n = P + N, [{}, {}], P // 4
    role = lambda e, i: i if e == 0 else P - 1 - i
    for e in range(N_ENVS):
        snake(d, e, P)
        for i in range(n):
            sel, stk, ful = role(e, i), role(e, n + i), role(e, 2 * n + i)
            typ, lvl = 13 + i % 3, 1 + i % 4
            _one_item(d, e, sel, typ, lvl, qty=3 + i % 9, price=2 + i % 9, ltick=sc.TICK - 1)
            _fill(d, e, stk, 11)
            _one_item(d, e, stk, typ, lvl, qty=1 + i % 5)
            _fill(d, e, ful, 12)
            d["ent"][e, F["gold"], stk] = d["ent"][e, F["gold"], ful] = 50 + i + e
            want[e][stk] = want[e][ful] = (sel, 0)
    for e in range(N_ENVS):
        sc._finish_items(d, e, P)
    acts = _buy_actions(d, P, want)

    def extra(pre, post, events, e, m, out):
        stackers = {role(e, n + i) for i in range(n)}
        assert {b for b, *_, s in out if s} == stackers, f"env {e}: exactly the stacking buyers succeed"
        freed = [row for b, _, row, _, s in out if s]
        assert m.freed == freed and len(freed) == n  # Buy order, not slot order
        by_slot = [row for b, _, row, _, s in sorted(out) if s]
        assert freed != by_slot, f"env {e}: Buy order equals slot order, the scenario shows nothing"
    return finish(cfg, d, P, S, acts, _buy_witness(P, acts, extra), items=False)


# ---------------------------------------------------------------- Give / GiveGold scenarios
def _give_witness(P, S, acts, extra, culled=None):
    def witness(pre, post, events):
        for e in range(N_ENVS):
            m = give_model(pre, e, P, S, acts[0])
            if culled:  # a player at health 0 leaves the realm at the tick's end: its items are destroyed
                m.freed += [it_row(w) for w in m.inv[culled[e]]]
                m.inv[culled[e]] = []
            m.assert_items(post, "give")
            m.assert_freed(pre, post, "give")
            m.assert_events(pre, events, (EV.GIVE_ITEM, EV.GIVE_GOLD), "give")
            extra(pre, post, events, e, m)
    return witness


def G1(P=128, N=256, preset="C4"):
    """All to one: P players on one tile, everyone else gives an unequipped item and gold to one
    receiver holding 9 items. The first three non-stacking gives in slot order land, every stacking
    one lands, the rest keep their item; the receiver's gold is the exact sum."""
    cfg, d = base(P, N, preset)
    S, recv = P + N, (0, 50)  # both among the first 100 datastore rows of the tile
    acts = noop(P)
    for e in range(N_ENVS):
        one_tile(d, e, range(P), ROW0 + 3 * e, 40 + 20 * e)
        _fill(d, e, recv[e], 8)
        _one_item(d, e, recv[e], 14, 3, qty=5)
        d["ent"][e, F["gold"], recv[e]] = 100 + e
        for p in range(P):
            if p == recv[e]:
                continue
            if (p + e) % 5 == 0:
                _one_item(d, e, p, 14, 3, qty=1 + p % 4)   # stacks onto the receiver's Arrows
            elif p % 7 == 6:
                _one_item(d, e, p, 14, 2, qty=2)           # same type, another level: no stack
            else:
                _one_item(d, e, p, 2 + p % 11, 1 + p % 9)
            d["ent"][e, F["gold"], p] = 10 + (p + e) % 13
    for e in range(N_ENVS):
        sc._finish_items(d, e, P)
        for p in range(P):
            if p != recv[e]:
                k = target_index(d, e, p, recv[e], S)
                acts[0, e, p, [H_GIVE, H_GIVET, H_GGP, H_GGT]] = [0, k, (p + e) % 9, k]

    def extra(pre, post, events, e, m):
        r = recv[e]
        givers = [p for p in range(P) if p != r]
        stack = [p for p in givers if (it_type(inv_of(pre, e, p)[0]), it_level(inv_of(pre, e, p)[0])) == (14, 3)]
        plain = [p for p in givers if p not in stack]
        landed = set(stack) | set(plain[:3])
        for p in givers:
            assert (len(inv_of(post, e, p)) == 0) == (p in landed), f"env {e}: giver {p}"
        assert len(inv_of(post, e, r)) == INV
        gold = int(pre["ent"][e, F["gold"], r]) + sum((p + e) % 9 + 1 for p in givers)
        assert int(post["ent"][e, F["gold"], r]) == gold, f"env {e}: receiver's gold"
        assert m.freed == [it_row(inv_of(pre, e, p)[0]) for p in stack], f"env {e}: freed rows in slot order"
        per = {}
        for ent_id, code, *_ in m.events:
            per.setdefault(ent_id, []).append(code)
        assert all(v in ([EV.GIVE_ITEM, EV.GIVE_GOLD], [EV.GIVE_GOLD]) for v in per.values())
    return finish(cfg, d, P, S, acts, _give_witness(P, S, acts, extra), items=False)


def G2(P=128, N=256, preset="C4"):
    """Chains on one tile: player i gives its item and its whole gold (amount == gold, the boundary
    of amount <= gold) to player i + 1; only the chain heads start with gold. Env 0 runs forward:
    every give follows the previous one and the gold ends at the chain's last player. Env 1 runs
    i -> i - 1: in slot order only the head's give finds gold. A Give target is one of the first 100
    entities of a tile, so the longest chain on one tile is 100 players; the others form a second
    chain on another tile."""
    cfg, d = base(P, N, preset)
    S = P + N
    acts = noop(P)
    chains = [list(range(0, min(P, 100))), list(range(100, P))]
    amount = (37, 99)
    for e in range(N_ENVS):
        for j, ch in enumerate(chains):
            if ch:
                one_tile(d, e, ch, ROW0 + 3 * e, 40 + 30 * j + 5 * e)
        for p in range(P):
            _one_item(d, e, p, 2 + (p + e) % 11, 1 + p % 9)
        for ch in chains:
            if ch:
                d["ent"][e, F["gold"], ch[0] if e == 0 else ch[-1]] = amount[e]
    for e in range(N_ENVS):
        sc._finish_items(d, e, P)
        for ch in chains:
            for i, p in enumerate(ch):
                j = i + 1 if e == 0 else i - 1
                if 0 <= j < len(ch):
                    k = target_index(d, e, p, ch[j], S)
                    acts[0, e, p, [H_GIVE, H_GIVET, H_GGP, H_GGT]] = [0, k, amount[e] - 1, k]

    def extra(pre, post, events, e, m):
        gold = post["ent"][e, F["gold"], :P].astype(np.int64)
        want = np.zeros(P, np.int64)
        for ch in chains:
            if ch:
                end = ch[-1] if e == 0 else (ch[-2] if len(ch) > 1 else ch[-1])
                want[end] = amount[e]
        assert np.array_equal(gold, want), f"env {e}: gold {np.flatnonzero(gold).tolist()}"
        n_gold = sum(1 for x in m.events if x[1] == EV.GIVE_GOLD)
        assert n_gold == (sum(max(len(ch) - 1, 0) for ch in chains) if e == 0 else sum(1 for ch in chains if len(ch) > 1))
    return finish(cfg, d, P, S, acts, _give_witness(P, S, acts, extra), items=False)


def G3(P=128, N=256, preset="C4"):
    """Three-party gives: the item goes to one player and the gold to another. Targets include a
    player with health 0 still in the realm and one on the next tile: both kinds fail."""
    cfg, d = base(P, N, preset)
    S = P + N
    acts = noop(P)
    n = 60
    dead, off = (7, 31), (8, 30)
    for e in range(N_ENVS):
        r, c = ROW0 + 4 * e, 50 + 9 * e
        one_tile(d, e, range(n), r, c)
        paint(d, e, r - 1, r + 1, c - 1, c + 2)
        d["ent"][e, F["col"], off[e]] = c + 1
        d["ent"][e, F["health"], dead[e]] = 0
        snake(d, e, P, row=ROW0 + 10, slots=range(n, P))
        for p in range(n):
            _fill(d, e, p, 1 + (p + e) % 11)
            d["ent"][e, F["gold"], p] = 5 + (p * 3 + e) % 40
    for e in range(N_ENVS):
        sc._finish_items(d, e, P)
        for p in range(n):
            if p == off[e]:
                continue
            t1, t2 = (p + 1 + e) % n, (p + 5) % n  # every residue: the dead one and the one next door too
            if t1 == p or t2 == p:
                continue
            acts[0, e, p, [H_GIVE, H_GIVET, H_GGP, H_GGT]] = [
                p % 3, target_index(d, e, p, t1, S), (p + e) % 7, target_index(d, e, p, t2, S)]

    def extra(pre, post, events, e, m):
        ids = {dead[e] + 1, off[e] + 1}
        assert not [x for x in m.events if x[6] in ids], f"env {e}: a give to the dead or the distant player"
        assert sum(1 for x in m.events if x[1] == EV.GIVE_ITEM) >= 16 and sum(1 for x in m.events if x[1] == EV.GIVE_GOLD) >= 16
        assert post["ent"][e, F["alive"], dead[e]] == 0
    return finish(cfg, d, P, S, acts, _give_witness(P, S, acts, extra, culled=dead), items=False)


# ---------------------------------------------------------------- Attack scenarios (equipment in A2 at C4 only)
def _set_skill(d, e, p, style, exp):
    d["ent"][e, F[STYLE_EXP[style]], p] = exp
    d["ent"][e, F[STYLE_LVL[style]], p] = level_of(exp)


def _attack_witness(P, S, acts, exchange, extra):
    def witness(pre, post, events):
        for e in range(N_ENVS):
            out = assert_attack(pre, post, events, e, P, S, acts[0], exchange, "attack")
            extra(pre, post, events, e, *out)
    return witness


def _gold(d, e, P, preset):
    if preset == "C4":
        d["ent"][e, F["gold"], :P] = [3 + (7 * p + 11 * e) % 50 for p in range(P)]


def A1(P=128, N=256, preset="C4", lethal=False):
    """Chain: along a snake slot s attacks slot s + 1 (P - 1 dependent attacks). Non-lethal: P - 1
    SCORE_HITs, each damage by SPEC §1 from the pre-state. `lethal`: every hit kills, so even slots
    kill odd slots and odd slots never act (no XP, no SCORE_HIT, no latest_combat_tick of their own)."""
    cfg, d = base(P, N, preset)
    S = P + N
    acts = noop(P)
    for e in range(N_ENVS):
        snake(d, e, P)
        _gold(d, e, P, preset)
        for p in range(P):
            _set_skill(d, e, p, p % 3, THRESH[(p + e) % 4])
            d["ent"][e, F["health"], p] = 3 if lethal else 60 + (p + e) % 40  # 3: the least damage (offense 15 / 4)
        for p in range(P - 1):
            acts[0, e, p, [H_ASTYLE, H_ATGT]] = [(p + e) % 3, target_index(d, e, p, p + 1, S)]

    def extra(pre, post, events, e, st, evs, executed, skipped):
        hits = [x for x in evs if x[1] == EV.SCORE_HIT]
        if not lethal:
            assert executed == list(range(P - 1)) and len(hits) == P - 1
            assert len({x[4] for x in hits}) > 1, "the chain's damages should differ"
        else:
            assert executed == list(range(0, P - 1, 2)) and skipped == list(range(1, P - 1, 2))
            ent = post["ent"][e]
            for p in range(1, P, 2):
                assert ent[F["alive"], p] == 0
                assert all(ent[F[k], p] == pre["ent"][e, F[k], p] for k in STYLE_EXP), f"env {e}: dead slot {p} gained XP"
    return finish(cfg, d, P, S, acts, _attack_witness(P, S, acts, preset == "C4", extra))


def A1_lethal(P=128, N=256, preset="C4"):
    return A1(P, N, preset, lethal=True)


A1_lethal.__doc__ = A1.__doc__


def A2(P=128, N=256, preset="C4"):
    """Focus fire: 44 attackers within L-inf <= 3 of one target whose health runs out at the k-th of
    them in slot order, 1 < k < 40: the later ones are skipped (no XP, no ammunition used), the kill,
    the gold and the loot go to k. Env 0: the victim's slot is below its attackers', it attacks first
    and its hit stands. Env 1: the victim's slot is above its killer's, its attack is dropped.
    With the Item system every attacker holds an equipped ammunition stack of its style, of quantity
    1 (the last unit: the row is freed iff the attack executes) or 2, and up to two more items; the
    victim holds three items, a Whetstone stack and an equipped last Arrow, which it fires in env 0
    and which is looted unfired in env 1. Without it (C3) nobody holds anything."""
    cfg, d = base(P, N, preset)
    S = P + N
    items = "Item" in cfg.systems
    acts = noop(P)
    n_att = 44
    victim = (0, 60)
    cells = [(dr, dc) for dr in range(-3, 4) for dc in range(-3, 4) if (dr, dc) != (0, 0)]
    info = []
    for e in range(N_ENVS):
        r, c = ROW0 + 2 + e, 40 + 30 * e
        paint(d, e, r - 4, r + 4, c - 4, c + 4)
        att = [p for p in range(1 + 9 * e, P) if p != victim[e]][:n_att]
        d["ent"][e, F["row"], victim[e]], d["ent"][e, F["col"], victim[e]] = r, c
        _set_skill(d, e, victim[e], 0, THRESH[9])  # defense 50: every hit is the floor, offense / 4
        for i, p in enumerate(att):
            dr, dc = cells[(i * 5 + e) % len(cells)]
            d["ent"][e, F["row"], p], d["ent"][e, F["col"], p] = r + dr, c + dc
            _set_skill(d, e, p, i % 3, THRESH[i % 3])
            if items:
                _fill(d, e, p, (i + e) % 3)
                _one_item(d, e, p, 13 + i % 3, 1, qty=1 + (i + e) % 2, eq=1)
        if items:
            _fill(d, e, victim[e], 3)
            _one_item(d, e, victim[e], 13, 1, qty=3)
            _one_item(d, e, victim[e], 14, 1, qty=1, eq=1)
        rest = [p for p in range(P) if p != victim[e] and p not in att]
        snake(d, e, P, row=ROW0 + 14, slots=rest)
        _gold(d, e, P, preset)
        d["ent"][e, F["health"], victim[e]] = 97
        d["ent"][e, F["health"], att] = 80
        for i, p in enumerate(att):
            acts[0, e, p, [H_ASTYLE, H_ATGT]] = [i % 3, target_index(d, e, p, victim[e], S)]
        acts[0, e, victim[e], [H_ASTYLE, H_ATGT]] = [1, target_index(d, e, victim[e], att[-1 - e], S)]
        info.append(att)

    def extra(pre, post, events, e, st, evs, executed, skipped, m=None):
        att, v = info[e], victim[e]
        kills = [x for x in evs if x[1] == EV.PLAYER_KILL]
        assert len(kills) == 1 and kills[0][6] == v + 1
        killer = kills[0][0] - 1
        k = att.index(killer) + 1
        assert 1 < k < 40, f"env {e}: the victim dies at attacker {k}"
        assert skipped == [p for p in att[k:]] + ([v] if v > killer else []), f"env {e}: skipped {skipped}"
        assert (v in executed) == (v < att[0]), f"env {e}: the victim's own attack"
        ent = post["ent"][e]
        for p in att[k:]:
            assert all(ent[F[x], p] == pre["ent"][e, F[x], p] for x in STYLE_EXP), f"env {e}: skipped attacker {p} gained XP"
        if preset == "C4":
            assert ent[F["gold"], killer] == pre["ent"][e, F["gold"], killer] + pre["ent"][e, F["gold"], v]
        if m is None:
            return
        # ammunition: a unit per executed attack and none for a skipped one, whatever the model says
        rows_of = lambda dd, p: {it_row(w) for w in inv_of(dd, e, p)}
        IC = INV * P
        n_freed = int(post["env"][e, E["item_free_count"]]) - int(pre["env"][e, E["item_free_count"]])
        tail = int(pre["env"][e, E["item_free_head"]]) + int(pre["env"][e, E["item_free_count"]])
        freed = [int(post["iring"][e, (tail + i) % IC]) for i in range(n_freed)]
        last = [p for p in att[k:] if any(it_eq(w) and it_qty(w) == 1 for w in inv_of(pre, e, p))]
        assert len(last) >= 8, f"env {e}: {len(last)} skipped attackers hold a last unit"
        for p in att[k:]:
            assert inv_of(post, e, p) == inv_of(pre, e, p), f"env {e}: skipped attacker {p} used ammunition"
            assert not rows_of(pre, p) & set(freed), f"env {e}: a row of skipped attacker {p} was freed"
        fired = []  # the rows of the last units fired by attackers 1..k, in slot order
        for p in ([v] if v in executed else []) + att[:k]:
            w = next(w for w in inv_of(pre, e, p) if it_eq(w))
            if it_qty(w) == 1:
                fired.append(it_row(w))
            else:
                w2 = next(x for x in inv_of(post, e, p) if it_row(x) == it_row(w))
                assert it_qty(w2) == it_qty(w) - 1, f"env {e}: attacker {p}'s ammunition"
        assert len(fired) >= 4 and [x for x in freed if x in fired] == fired, f"env {e}: last units fired"
        # loot: every item the victim still held goes to k, LOOT_ITEM at k only, victim inventory order
        held = [w for w in inv_of(pre, e, v) if it_row(w) not in fired]
        assert len(held) == (4 if v in executed else 5)
        ev = events[e]
        loot = ev[ev[:, C["event"]] == EV.LOOT_ITEM]
        assert loot[:, C["ent_id"]].tolist() == [killer + 1] * len(held), f"env {e}: LOOT_ITEM not at the killer"
        assert [(int(x[4]), int(x[5]), int(x[6])) for x in loot] == [(it_type(w), it_level(w), it_qty(w)) for w in held]
        vrows = {it_row(w) for w in held}
        assert not post["items"][e, v].any()
        assert all(not rows_of(post, p) & vrows for p in range(P) if p != killer), f"env {e}: loot outside the killer"
        assert (rows_of(post, killer) | set(freed)) >= vrows and rows_of(post, killer) & vrows
        assert freed == m.freed

    if items:
        return finish(cfg, d, P, S, acts, _combat_witness(
            P, S, acts, [(), ()], lambda pre, post, events, e, st, m, evs, executed, skipped:
            extra(pre, post, events, e, st, evs, executed, skipped, m)))
    return finish(cfg, d, P, S, acts, _attack_witness(P, S, acts, False, extra))


def A3(P=128, N=256, preset="C4"):
    """Thresholds: attackers with style exp 6 below a level threshold (LEVEL_UP fires) and exactly at
    one (it does not); one at level 10 with exp far above 8,000 stays at 10; targets at L-inf exactly
    3 (hit) and 4 (out of reach); targets with time_alive 18 and 19, 19 and 20 after the update
    phase (immune, not immune)."""
    cfg, d = base(P, N, preset)
    S, n = P + N, P // 2
    acts = noop(P)
    kinds = []
    top = max(i for i in range(n) if i % 5 != 3 and i % 7 not in (2, 5))  # its attack executes
    for e in range(N_ENVS):
        r = ROW0 + 2 * e
        paint(d, e, r - 1, r + 5)
        ks = []
        for i in range(n):
            a, t = (2 * i, 2 * i + 1) if e == 0 else (2 * i + 1, 2 * i)
            style, j = i % 3, 1 + i % 9
            below = (i // 9) % 2 == 0
            exp = THRESH[j] - 6 if below else THRESH[j]
            if i == top:
                exp, below = 20000, False
            _set_skill(d, e, a, style, exp)
            dist = 4 if i % 5 == 3 else 3
            alive = 18 if i % 7 == 2 else 19 if i % 7 == 5 else 30
            c = (16 + 2 * i) if e == 0 else (142 - 2 * i)
            d["ent"][e, F["row"], a], d["ent"][e, F["col"], a] = r, c
            d["ent"][e, F["row"], t], d["ent"][e, F["col"], t] = r + dist, c
            d["ent"][e, F["time_alive"], t] = alive
            ks.append((a, t, style, below, dist, alive))
        for a, t, style, *_ in ks:
            acts[0, e, a, [H_ASTYLE, H_ATGT]] = [style, target_index(d, e, a, t, S)]
        kinds.append(ks)

    def extra(pre, post, events, e, st, evs, executed, skipped):
        ups = {x[0] - 1 for x in evs if x[1] == EV.LEVEL_UP}
        want_exec = [a for a, t, s, below, dist, alive in kinds[e] if dist == 3 and alive != 18]
        assert sorted(executed) == sorted(want_exec), f"env {e}: executed attacks"
        assert ups == {a for a, t, s, below, dist, alive in kinds[e] if below and a in want_exec}, f"env {e}: LEVEL_UPs"
        assert len(ups) >= 8 and len(want_exec) - len(ups) >= 8
        a10, _, s10, *_ = kinds[e][top]
        assert a10 in executed and post["ent"][e, F[STYLE_LVL[s10]], a10] == 10 and post["ent"][e, F[STYLE_EXP[s10]], a10] == 20006
        for a, t, s, below, dist, alive in kinds[e]:
            assert post["ent"][e, F["time_alive"], t] == alive + 1
    return finish(cfg, d, P, S, acts, _attack_witness(P, S, acts, preset == "C4", extra))


def A6(P=128, N=256, preset="C4"):
    """Mutual lethal attacks, P / 2 pairs on a snake: the lower slot kills, the higher never acts."""
    cfg, d = base(P, N, preset)
    S = P + N
    acts = noop(P)
    for e in range(N_ENVS):
        snake(d, e, P)
        _gold(d, e, P, preset)
        d["ent"][e, F["health"], :P] = 3  # the least damage (offense 15 / 4)
        for p in range(P):
            _set_skill(d, e, p, (p + e) % 3, THRESH[p % 3])
            acts[0, e, p, [H_ASTYLE, H_ATGT]] = [(p + e) % 3, target_index(d, e, p, p ^ 1, S)]

    def extra(pre, post, events, e, st, evs, executed, skipped):
        assert executed == list(range(0, P, 2)) and skipped == list(range(1, P, 2))
        assert np.array_equal(post["ent"][e, F["alive"], :P], np.arange(P) % 2 == 0)
        assert np.all(post["ent"][e, F["player_kills"], 0:P:2] == 1)
    return finish(cfg, d, P, S, acts, _attack_witness(P, S, acts, preset == "C4", extra))


def _combat_witness(P, S, acts, npc_attacks, extra):
    def witness(pre, post, events):
        for e in range(N_ENVS):
            out = assert_combat(pre, post, events, e, P, S, acts[0], npc_attacks[e], "combat")
            extra(pre, post, events, e, *out)
    return witness


def A4(P=128, N=256, preset="C4"):
    """Ammunition and loot order, groups of four slots (a, b, c, d) along a snake, four kinds:
    0: a (12 items, equipped Whetstones x2) kills b (12 items): 12 rows freed, 12 LOOT_ITEM; c fires
       its last Arrow at d (its row is freed, no kill);
    1: a (12 items, its last equipped Whetstone) kills b (12 items): a's row first, then b's first
       item fits and the other 11 rows are freed;
    2: a fires its last Rune at b and is then killed by b (a victim that fired before dying); b
       holds 11 items with an Arrow stack that a's Arrows join, one more item fits, the rest go;
    3: a fires one of two Whetstones at b; c (2 items) kills and loots d (3 items): all fit.
    The free ring's tail is the serial slot-order sequence (the shooter's row, then its loot's rows),
    LOOT_ITEM events per killer in slot order after every attack event, gold moves to the killer."""
    cfg, d = base(P, N, preset)
    S = P + N
    acts = noop(P)
    plan = [[], []]
    for e in range(N_ENVS):
        snake(d, e, P)
        d["ent"][e, F["gold"], :P] = [2 + (5 * p + 3 * e) % 40 for p in range(P)]
        for i in range(P // 4):
            a, b, c, dd = range(4 * i, 4 * i + 4)
            kind = (i + e) % 4
            if kind == 0:
                _fill(d, e, a, 11)
                _one_item(d, e, a, 13, 1, qty=2, eq=1)
                _fill(d, e, b, 12)
                _one_item(d, e, c, 14, 1, qty=1, eq=1)
                d["ent"][e, F["health"], b] = 3
                plan[e] += [(a, 0, b), (c, 1, dd)]
            elif kind == 1:
                _fill(d, e, a, 11)
                _one_item(d, e, a, 13, 1, qty=1, eq=1)
                _fill(d, e, b, 12)
                d["ent"][e, F["health"], b] = 3
                plan[e] += [(a, 0, b)]
            elif kind == 2:
                _one_item(d, e, a, 15, 1, qty=1, eq=1)
                _one_item(d, e, a, 14, 2, qty=4)
                _fill(d, e, a, 5)
                _fill(d, e, b, 10)
                _one_item(d, e, b, 14, 2, qty=6)
                d["ent"][e, F["health"], a] = 3
                plan[e] += [(a, 2, b), (b, i % 3, a)]
            else:
                _one_item(d, e, a, 13, 1, qty=2, eq=1)
                _fill(d, e, c, 2)
                _fill(d, e, dd, 3)
                d["ent"][e, F["health"], dd] = 3
                plan[e] += [(a, 0, b), (c, 1, dd)]
    for e in range(N_ENVS):
        sc._finish_items(d, e, P)
        for x, sty, t in plan[e]:
            acts[0, e, x, [H_ASTYLE, H_ATGT]] = [sty, target_index(d, e, x, t, S)]

    def extra(pre, post, events, e, st, m, evs, executed, skipped):
        assert sorted(executed) == sorted(x for x, _, _ in plan[e]) and not skipped
        n_kind = {k: sum(1 for i in range(P // 4) if (i + e) % 4 == k) for k in range(4)}
        loot = [x for x in evs if x[1] == EV.LOOT_ITEM]
        assert len(loot) == 12 * n_kind[0] + 12 * n_kind[1] + 4 * n_kind[2] + 3 * n_kind[3]
        assert [x[0] for x in loot] == sorted(x[0] for x in loot), "LOOT_ITEM per killer in slot order"
        assert len(m.freed) == 13 * n_kind[0] + 12 * n_kind[1] + 4 * n_kind[2], f"env {e}: {len(m.freed)} rows freed"
        assert evs.index(loot[0]) > max(i for i, x in enumerate(evs) if x[1] == EV.SCORE_HIT)
    return finish(cfg, d, P, S, acts, _combat_witness(P, S, acts, [(), ()], extra), items=False)


def A5(P=128, N=256, preset="C4"):
    """NPCs. A player holding 11 items kills an NPC: the armor piece fits, the tool is destroyed, two
    LOOT_ITEM events either way, the NPC's gold moves. A hostile NPC kills a player with a full
    inventory: the items are destroyed, their rows freed in the cull, nothing is looted."""
    cfg, d = base(P, N, preset)
    S = P + N
    acts = noop(P)
    npc_attacks = [[], []]
    hunters, preys = (2, 9), (5, 3)
    for e in range(N_ENVS):
        row = snake(d, e, P, row=ROW0 + 8)
        r = ROW0 + 2 * e
        paint(d, e, r - 2, r + 2, 30, 60)
        ent = d["ent"][e]
        assert ent[F["alive"], P] and ent[F["alive"], P + 1], "the reset state holds at least two NPCs"
        assert abs(row - r) > 7
        h, q, n1, n2 = hunters[e], preys[e], P, P + 1
        ent[F["row"], h], ent[F["col"], h] = r, 35 + e
        ent[F["row"], n1], ent[F["col"], n1] = r, 37 + e  # two tiles from its hunter
        ent[F["row"], q], ent[F["col"], q] = r, 52 + e
        ent[F["row"], n2], ent[F["col"], n2] = r + 1, 52 + e  # next to its prey: it stays and attacks
        for f, v in dict(health=1, gold=7 + e, npc_type=1, npc_level=3 + e, drop_armor=e, drop_tool=2 + e,
                         equip_defense=2, target_id=0, attacker_id=0).items():
            ent[F[f], n1] = v
        for f, v in dict(health=100, npc_type=3, target_id=q + 1, attacker_id=0, style=e, equip_offense=9).items():
            ent[F[f], n2] = v
        ent[F["health"], q] = 6
        ent[F["gold"], :P] = [1 + (3 * p + e) % 20 for p in range(P)]
        _fill(d, e, h, 11)
        _fill(d, e, q, 12)
        npc_attacks[e] = [(n2, q)]
    for e in range(N_ENVS):
        sc._finish_items(d, e, P)
        acts[0, e, hunters[e], [H_ASTYLE, H_ATGT]] = [e, target_index(d, e, hunters[e], P, S)]

    def extra(pre, post, events, e, st, m, evs, executed, skipped):
        h, q = hunters[e], preys[e]
        assert executed == [h, P + 1] and not skipped
        loot = [x for x in evs if x[1] == EV.LOOT_ITEM]
        assert [(x[0], x[2], x[3]) for x in loot] == [(h + 1, 2 + e, 3 + e), (h + 1, 8 + 2 + e, 3 + e)]
        inv = inv_of(post, e, h)
        assert len(inv) == INV and sum(1 for w in inv if (it_type(w), it_level(w)) == (2 + e, 3 + e)) >= 1 and m.taken == 1
        assert post["ent"][e, F["gold"], h] == pre["ent"][e, F["gold"], h] + 7 + e
        assert m.freed == [it_row(w) for w in inv_of(pre, e, q)] and not post["items"][e, q].any()
        assert post["ent"][e, F["alive"], q] == 0 and post["ent"][e, F["gold"], q] == pre["ent"][e, F["gold"], q]
    return finish(cfg, d, P, S, acts, _combat_witness(P, S, acts, npc_attacks, extra), items=False)


# ---------------------------------------------------------------- whole-env scenarios
def M1(P=128, N=256, preset="C4"):
    """Mass death: food = water = 0, health 10, not resilient, 12 items each: P deaths in one tick,
    the maximum of all three fields of the cull scan. P AGENT_CULLED in slot order, item_free_count
    12 P with the rows in slot, then inventory order, done, everyone terminated with reward -1 and
    nobody truncated; the second tick is the auto-reset."""
    cfg, d = base(P, N, preset)
    S = P + N
    for e in range(N_ENVS):
        snake(d, e, P)
        ent = d["ent"][e]
        ent[F["food"], :P] = ent[F["water"], :P] = 0
        ent[F["health"], :P] = 10
        ent[F["resilient"], :P] = 0
        ent[F["gold"], :P] = [(p + e) % 30 for p in range(P)]
        for p in range(P):
            _fill(d, e, p, INV)
    acts = noop(P)

    def witness(pre, post, events):
        for e in range(N_ENVS):
            env = post["env"][e]
            assert env[E["players_alive"]] == 0 and env[E["done"]] == 1
            assert not post["ent"][e, F["alive"], :P].any()
            assert env[E["item_free_count"]] == INV * P and not post["items"][e].any()
            m = Model(pre, e, P)
            m.freed = [it_row(w) for p in range(P) for w in inv_of(pre, e, p)]
            m.assert_freed(pre, post, "cull")
            assert_events(pre, events, e, (EV.AGENT_CULLED,), [(p + 1, EV.AGENT_CULLED, 0, 0, 0, 0, 0) for p in range(P)], "cull")
            ring = [int(post["ring"][e, (int(pre["env"][e, E["free_head"]]) + int(pre["env"][e, E["free_count"]]) + i) % S])
                    for i in range(P)]
            assert ring == pre["ent"][e, F["ds_row"], :P].tolist(), f"env {e}: datastore rows freed in slot order"
    witness.outputs = lambda rew, term, trunc, mask: (
        np.all(rew == -1.0) and np.all(term == 1) and not trunc.any() and np.all(mask == 1))
    witness.auto_reset = True
    return finish(cfg, d, P, S, acts, witness)


def M2(P=128, N=256, preset="C4", event_cap=4096):
    """Everyone moves onto a tile that is a new exploration record and lists an item in one tick: the
    Move / Sell packed scan at P | P. All GO_FARTHEST events come before all LIST_ITEM events, each
    group in slot order; with event_cap 64 and 100 the ring wraps inside the tick (power-of-two and
    modulo paths) and holds the last event_cap rows."""
    cfg, d = base(P, N, preset, event_cap=event_cap)
    S = P + N
    acts = noop(P)
    rows = []
    for e in range(N_ENVS):  # two rows of P / 2 (column 16 or 143 is 64 tiles from the centre: no record there)
        r = ROW0 + 6 * e
        paint(d, e, r - 1, r + 3)
        for p in range(P):
            d["ent"][e, F["row"], p] = r + 2 * (p % 2)
            d["ent"][e, F["col"], p] = 17 + p // 2 if e == 0 else 142 - p // 2
        rows.append(d["ent"][e, F["row"], :P].astype(np.int64))
        d["ent"][e, F["exploration"], :P] = 0
        for p in range(P):
            _fill(d, e, p, 1 + (p + e) % 3)
            acts[0, e, p, [H_MOVE, H_SELL, H_SELLP]] = [1 - e, (p + e) % 2 if (p + e) % 3 else 0, (3 * p + e) % 99]

    def witness(pre, post, events):
        for e in range(N_ENVS):
            ent = pre["ent"][e]
            nr = rows[e] + (1 if e == 0 else -1)
            want = [(p + 1, EV.GO_FARTHEST, 0, 0, 64 - max(abs(int(nr[p]) - 80), abs(int(ent[F["col"], p]) - 80)), 0, 0) for p in range(P)]
            assert all(x[4] > 0 for x in want)
            for p in range(P):
                w = inv_of(pre, e, p)[acts[0, e, p, H_SELL]]
                want.append((p + 1, EV.LIST_ITEM, it_type(w), it_level(w), it_qty(w), int(acts[0, e, p, H_SELLP]) + 1, 0))
            n0 = int(pre["env"][e, E["event_count"]])
            ev = events[e]
            ev = ev[ev[:, C["tick"]] == pre["env"][e, E["tick"]] + 1]
            ev = ev[np.isin(ev[:, C["event"]], (EV.GO_FARTHEST, EV.LIST_ITEM))]
            keep = min(len(want), event_cap)
            got = [tuple(int(x) for x in r[[1, 3, 4, 5, 6, 7, 8]]) for r in ev]
            assert got[-keep:] == want[-keep:] and len(got) >= keep, f"env {e}: Move / Sell events"
            assert post["env"][e, E["event_count"]] == n0 + 2 * P
            assert np.all(post["ent"][e, F["row"], :P] == nr)
            for p in range(P):
                k = acts[0, e, p, H_SELL]
                assert it_price(inv_of(post, e, p)[k]) == acts[0, e, p, H_SELLP] + 1
    return finish(cfg, d, P, S, acts, witness)


def M2_cap64(P=128, N=256, preset="C4"):
    return M2(P, N, preset, event_cap=64)


def M2_cap100(P=128, N=256, preset="C4"):
    return M2(P, N, preset, event_cap=100)


M2_cap64.__doc__ = M2_cap100.__doc__ = M2.__doc__


def H1_one_tile(P=128, N=256, preset="C4"):
    """P players on one Foilage tile: only the lowest slot eats, the tile is Scrub afterwards (the
    tile is one whose bank material is Grass, so the map step of the same tick cannot respawn it)."""
    cfg, d = base(P, N, preset)
    S = P + N
    bank = make_oracle(cfg).map_bank()
    pos = []
    for e in range(N_ENVS):
        r = ROW0 + 3 * e
        c = next(c for c in range(45 + 17 * e, 120) if bank[d["env"][e, E["map_id"]], r, c] == GRASS)
        one_tile(d, e, range(P), r, c)
        d["mat"][e, r, c] = FOILAGE
        d["ent"][e, F["food"], :P] = [20 + (p + e) % 30 for p in range(P)]
        pos.append((r, c))

    def witness(pre, post, events):
        for e in range(N_ENVS):
            assert_events(pre, events, e, (EV.EAT_FOOD,), [(1, EV.EAT_FOOD, 0, 0, 0, 0, 0)], "harvest")
            food = pre["ent"][e, F["food"], :P] - 5
            food[0] = 100
            assert np.array_equal(post["ent"][e, F["food"], :P], food)
            assert pre["mat"][e][pos[e]] == FOILAGE and post["mat"][e][pos[e]] == SCRUB, f"env {e}: the tile is not depleted"
    return finish(cfg, d, P, S, noop(P), witness)


def H1_distinct(P=128, N=256, preset="C4"):
    """P players on P distinct Foilage tiles: the position hash at its fullest, everyone eats."""
    cfg, d = base(P, N, preset)
    S = P + N
    for e in range(N_ENVS):
        row = snake(d, e, P)
        paint(d, e, row, row, m=FOILAGE)
        d["ent"][e, F["food"], :P] = [20 + (p + e) % 30 for p in range(P)]

    def witness(pre, post, events):
        for e in range(N_ENVS):
            assert_events(pre, events, e, (EV.EAT_FOOD,), [(p + 1, EV.EAT_FOOD, 0, 0, 0, 0, 0) for p in range(P)], "harvest")
            assert np.all(post["ent"][e, F["food"], :P] == 100)
    return finish(cfg, d, P, S, noop(P), witness)


def H1_professions(P=128, N=256, preset="C4"):
    """Professions: players with 10, 11 and 12 items adjacent to Fish and standing on Ore in one tick,
    and the 12-item case whose on-tile harvest stacks. Rows are allocated from the free ring in slot
    order, the ration before the on-tile Whetstone; what does not fit is dropped."""
    cfg, d = base(P, N, preset)
    S, n = P + N, 24
    for e in range(N_ENVS):
        row = ROW0 + 6 * e
        paint(d, e, row - 1, row + 1)
        snake(d, e, P, row=ROW0 + 12, slots=range(n, P))
        for i in range(n):
            p = i if e == 0 else n - 1 - i
            c = 20 + 3 * i
            d["ent"][e, F["row"], p], d["ent"][e, F["col"], p] = row, c
            d["mat"][e, row, c], d["mat"][e, row - 1, c] = ORE, FISH
            kind = i % 4
            _fill(d, e, p, (10, 11, 12, 11)[kind])
            if kind == 3:
                _one_item(d, e, p, 13, 1, qty=4)  # 12 items, the Whetstone L1 stacks

    def witness(pre, post, events):
        for e in range(N_ENVS):
            m = Model(pre, e, P)
            IC = INV * P
            head = int(pre["env"][e, E["item_free_head"]])
            taken = 0
            for p in range(n):
                for typ in (16, 13):  # the ration, then the on-tile Whetstone, both level 1 without tools
                    m.log(p, EV.HARVEST_ITEM, typ, 1, 1)
                    k = m.stack_slot(p, [w0(typ, 1), 1])
                    if k >= 0:
                        m.inv[p][k][1] += 1
                    elif len(m.inv[p]) < INV:
                        row = int(pre["iring"][e, (head + taken) % IC])
                        taken += 1
                        m.inv[p].append([w0(typ, 1), 1 | row << 16])
                        m.inv[p].sort(key=it_row)
            m.assert_items(post, "harvest")
            m.assert_events(pre, events, (EV.HARVEST_ITEM,), "harvest")
            assert post["env"][e, E["item_free_head"]] == (head + taken) % IC
            assert post["env"][e, E["item_free_count"]] == pre["env"][e, E["item_free_count"]] - taken
            assert np.all(post["ent"][e, F["fishing_exp"], :n] == 30) and np.all(post["ent"][e, F["prospecting_exp"], :n] == 15)
    return finish(cfg, d, P, S, noop(P), witness)


# ---------------------------------------------------------------- the case list
BUY = (B1, B2, B3, B3_full, B4, B5)
GIVE = (G1, G2, G3)
ATTACK = (A1, A1_lethal, A2, A3, A6)
LOOT = (A4, A5)  # ammunition, loot, NPCs: every system on
WHOLE = (M1, M2, M2_cap64, M2_cap100, H1_one_tile, H1_distinct, H1_professions)
SMALL = (B1, G1, A1, M1)  # again at P = 100, N = 50: the generic kernel, S no multiple of 8


def cases():
    """[(id, builder, P, N, preset)]: everything at C4 128 / 256 (tick_kernel<ALL, 384, 128>), the
    Attack scenarios at C3 too (tick_kernel_w8<C3, 384, 128>, the slim entity table), and B1, G1, A1,
    M1 at 100 / 50 (the generic kernel, a partial wave)."""
    out = [(f"{f.__name__}-C4-128", f, 128, 256, "C4") for f in BUY + GIVE + ATTACK + LOOT + WHOLE]
    out += [(f"{f.__name__}-C3-128", f, 128, 256, "C3") for f in ATTACK]
    out += [(f"{f.__name__}-C4-100", f, 100, 50, "C4") for f in SMALL]
    return out


def make_oracle(cfg):
    return sc.make_oracle(cfg)


def run(handle_step, get_state, get_events, blob, acts, P, S, witness):
    """Drive `acts` through a handle whose state was set to `blob`: the witness on the state after
    the first tick, check_invariants on the state and the event log after every tick; returns the
    post-state dict of the last tick."""
    pre = split_state(blob, N_ENVS, S, P)
    post = None
    for t in range(acts.shape[0]):
        handle_step(acts[t])
        post = split_state(get_state(), N_ENVS, S, P)
        events = [get_events(e) for e in range(N_ENVS)]
        if t == 0:
            witness(pre, post, events)
        check_invariants(post, P, S, events)
    return post
