"""Scenario builders for the obs, wire and market kernels' saturation and threshold states.

The obs kernels branch on per-row counts (visible entities nv, listings nm, the inventory prefix
ninv, the remembered zero thresholds hv / hm) that scripted rollouts never push to the values
where the code changes path. Here those states are built directly: every builder takes a state
blob derived from a reset C4 blob (MAP_N=4, early_stop_agent_num=0, N_ENVS envs; tick set to TICK by
`reset_blob`) and returns a new valid blob -- unique item rows in 1..12P, the item free ring
consistent with them, compact inventories, positions inside the map interior. `schedule()` is the
fixed transition schedule tests/test_obs_scenarios.py (CPU: the schedule reaches what it claims)
and tests/test_gpu_obs_saturation.py (HIP vs oracle) walk; the numpy restatements at the end
(window_ids, priced_rows, buy_bits, wire_expect) are computed from the blob alone, never from an
obs. Not a conftest: a plain module the two tests import."""

from __future__ import annotations

import numpy as np

from nmmo_amd import abi
from oracle import wire as owire
from oracle.oracle import OracleEnvs, join_state, split_state

N_ENVS = 2
TICK = 3            # CurrentTick of every scenario state (nonzero; listings are 1..3 ticks old)
N_TASKS = 131       # > PLAYER_N: a distinct task index per player
BLOCK_W = 12        # crowd(): players packed 12 per row -- 128 players fill 12 x 11 < 15 x 15
IMPASSABLE = (0, 1, 5, 14, 15)  # common.h Material: void, water, stone, ocean, fish
LISTING_COUNTS = (0, 1, 24, 25, 88, 89, 255, 256, 257, 960, 961, 1023, 1024, 1536)
GOLD = (0, 3, 10, 30, 45, 60, 89, 90, 95)  # straddles the prices 1..90
E, F = abi.E, abi.F
INV = abi.INV_SLOTS
AMMO = (13, 14, 15)


def config(P: int = 128, N: int = 256, **kw):
    from nmmo_amd.config import Config

    return Config.preset("C4", MAP_N=4, early_stop_agent_num=0, PLAYER_N=P, NPC_N=N, **kw)


def task_table():
    """N_TASKS TickGE tasks with distinct fp16 embeddings (the Task obs differs per task index)."""
    from nmmo_amd import tasks as T

    rng = np.random.default_rng(5)
    tl = [T.task("TickGE", num_tick=20 + i) for i in range(N_TASKS)]
    emb = rng.standard_normal((N_TASKS, 2048)).astype(np.float16)
    return tl, emb


def base_assign(P: int) -> np.ndarray:
    return np.tile(np.arange(P, dtype=np.int32) % N_TASKS, (N_ENVS, 1))


def set_tasks(handle, P: int):
    """The scenarios' task table on an OracleEnvs or an NmmoEngine (before any set_state)."""
    tl, emb = task_table()
    handle.set_tasks(tl, emb, base_assign(P))


def make_oracle(cfg, seed: int = 17) -> OracleEnvs:
    orc = OracleEnvs(cfg, N_ENVS, seed=seed)
    set_tasks(orc, orc.P)
    return orc


def reset_blob(cfg, seed: int = 17) -> np.ndarray:
    """The reset state every scenario starts from, its tick moved to TICK."""
    orc = make_oracle(cfg, seed)
    orc.reset()
    d = split_state(orc.get_state(), N_ENVS, orc.S, orc.P)
    d["env"][:, E["tick"]] = TICK
    P = orc.P  # every other player past its spawn immunity: Attack.Target bits of both kinds
    d["ent"][:, F["time_alive"], :P] = np.where(np.arange(P) % 2, 30, 5)
    return join_state(d)


# ---------------------------------------------------------------- item bookkeeping
def _w0(typ, lvl, eq=0, price=0, ltick=0):
    return typ | lvl << 5 | eq << 9 | price << 10 | ltick << 17


def _equip_slot(typ):
    return {2: 0, 3: 1, 4: 2}.get(typ, 3 if 5 <= typ <= 12 else 4 if typ in AMMO else -1)


def _item_type(e, p, k):
    """Slot k's type: 3 is coprime to 16, so an inventory's 12 types are distinct (no two
    ammunition stacks of one type) and 11 slots or more hold nearly every type."""
    return 2 + (p * 5 + k * 3 + e) % 16


def _new_item(e, p, k):
    typ = _item_type(e, p, k)
    qty = 1 + (p * 3 + k) % 40 if typ in AMMO else 1
    return [_w0(typ, 1 + (p + k) % 9), qty]


def _ninv(items_p) -> int:
    occ = (items_p[:, 0] & 31) != 0
    n = int(occ.sum())
    assert occ[:n].all(), "inventory has a hole"
    return n


def _finish_items(d, e, P):
    """Unique item rows (a pseudo-random subset of 1..12P, ascending inside each inventory as the
    tick keeps them, owners interleaved so the Market's row order is not the owner order), the item
    free ring holding exactly the other rows, and item_level = the equipped items' levels."""
    it = d["items"][e]
    n_inv = [_ninv(it[p]) for p in range(P)]
    n, IC = sum(n_inv), INV * P
    rng = np.random.default_rng(1000 + 7 * n + e)
    rows = rng.permutation(IC)[:n] + 1
    i = 0
    for p in range(P):
        k = n_inv[p]
        r = np.sort(rows[i:i + k]).astype(np.uint32)
        it[p, :k, 1] = (it[p, :k, 1] & 0xFFFF) | (r << 16)
        i += k
        eq = ((it[p, :k, 0] >> 9) & 1) != 0
        d["ent"][e, F["item_level"], p] = int(((it[p, :k, 0] >> 5) & 15)[eq].sum())
    free = np.setdiff1d(np.arange(1, IC + 1), rows)
    d["iring"][e, :] = 0
    d["iring"][e, :free.size] = free
    d["env"][e, E["item_free_head"]] = 0
    d["env"][e, E["item_free_count"]] = free.size


def _edit(builder):
    """blob -> blob over the chosen envs (default: all), dimensions from P and S."""
    def run(blob, *args, envs=None, P=128, S=384):
        d = split_state(blob, N_ENVS, S, P)
        for e in (range(N_ENVS) if envs is None else envs):
            builder(d, e, P, S, *args)
        return join_state(d)
    run.__name__, run.__doc__ = builder.__name__.lstrip("_"), builder.__doc__
    return run


# ---------------------------------------------------------------- builders
def _block_origin(mat, e):
    """Top-left of the (BLOCK_W + 1)-row, BLOCK_W-column region with the fewest impassable tiles,
    every window of it inside the map interior's vision margin."""
    bad = np.isin(mat, IMPASSABLE).astype(np.int32)
    ii = np.pad(bad.cumsum(0).cumsum(1), ((1, 0), (1, 0)))
    h, w = BLOCK_W + 1, BLOCK_W
    cnt = ii[h:, w:] - ii[:-h, w:] - ii[h:, :-w] + ii[:-h, :-w]
    lo, hi = 16 + 8, 143 - 8 - h
    sub = cnt[lo:hi, lo:hi]
    order = np.argsort(sub, axis=None, kind="stable")
    r, c = np.unravel_index(order[e * 37], sub.shape)  # another block per env
    return int(r) + lo, int(c) + lo


def _crowd(d, e, P, S, k):
    """The first k players packed BLOCK_W per row into a block smaller than one 15x15 window, and
    up to 8 live NPCs in the row above it, so a window mixes player and NPC datastore rows. From
    k = 3 the last of them shares a tile with another (Give / GiveGold targets). With 128 players
    an agent sees 64..100 entities, the middle ones with more than 100 in window."""
    assert 1 <= k <= P
    ent = d["ent"][e]
    r0, c0 = _block_origin(d["mat"][e], e)
    for i in range(k):
        ent[F["row"], i], ent[F["col"], i] = r0 + 1 + i // BLOCK_W, c0 + i % BLOCK_W
    if k >= 3:  # one pair on one tile: Give / GiveGold targets
        ent[F["row"], k - 1], ent[F["col"], k - 1] = ent[F["row"], (k - 1) // 2], ent[F["col"], (k - 1) // 2]
    npcs = [s for s in range(P, S) if ent[F["alive"], s]][:min(8, k // 2)]
    for j, s in enumerate(npcs):
        ent[F["row"], s], ent[F["col"], s] = r0, c0 + j


def _inventories(d, e, P, S, kind):
    """kind "mixed": ninv in {0, 1, 11, 12} across agents, level-1 equipped items (one per
    equipment slot at the most), ammunition stacks and every item type; "full": 12 unequipped
    items each (all of them can be listed); "empty": none."""
    it = d["items"][e]
    it[:] = 0
    for p in range(P):
        n = {"mixed": (0, 1, 11, 12)[(p + e) % 4], "full": INV, "empty": 0}[kind]
        used = set()
        for k in range(n):
            it[p, k] = _new_item(e, p, k)
            slot = _equip_slot(_item_type(e, p, k))
            if kind == "mixed" and (p + k) % 3 == 0 and slot not in used:
                used.add(slot)
                it[p, k, 0] = _w0(_item_type(e, p, k), 1, eq=1)
    _finish_items(d, e, P)


def _listings(d, e, P, S, m):
    """Exactly m priced items, spread over owners and slots (inventories of players in the realm are
    topped up with unequipped items first when fewer than m could be listed): prices 1..90,
    listed 1..3 ticks ago, and gold per agent straddling the prices."""
    it, ent = d["items"][e], d["ent"][e]
    assert 0 <= m <= INV * P
    it[:, :, 0] &= 0x3FF  # unlist everything
    n_inv = [_ninv(it[p]) for p in range(P)]
    live = [p for p in range(P) if ent[F["alive"], p]]

    def cands():
        return [(p, k) for p in live for k in range(n_inv[p]) if not (it[p, k, 0] >> 9) & 1]

    c = cands()
    while len(c) < m:  # a round of one more item per player with room
        room = [p for p in live if n_inv[p] < INV]
        assert room, "more listings than unequipped slots"
        for p in room[:m - len(c)]:
            it[p, n_inv[p]] = _new_item(e, p, n_inv[p])
            n_inv[p] += 1
        c = cands()
    pick = np.random.default_rng(77 + 3 * m + e).permutation(len(c))[:m]
    for j in pick:
        p, k = c[j]
        it[p, k, 0] |= (1 + (p * 7 + k * 13 + e * 5) % 90) << 10 | (TICK - 1 - (p + k) % 3) << 17
    ent[F["gold"], :P] = [GOLD[(p + e) % len(GOLD)] for p in range(P)]
    _finish_items(d, e, P)


def _out_of_realm(d, e, P, S, players):
    """The chosen players leave the realm as the tick's cull leaves them: alive and health 0,
    died at TICK, their datastore row on the entity free ring, their items destroyed."""
    ent, env, ring = d["ent"][e], d["env"][e], d["ring"][e]
    for p in players:
        if not ent[F["alive"], p]:
            continue
        ring[(env[E["free_head"]] + env[E["free_count"]]) % S] = ent[F["ds_row"], p]
        env[E["free_count"]] += 1
        env[E["players_alive"]] -= 1
        ent[F["alive"], p] = ent[F["health"], p] = 0
        ent[F["died_tick"], p] = TICK
        d["items"][e, p] = 0
    _finish_items(d, e, P)


def _task_swap(d, e, P, S, shift=17):
    """Another task index per player (still distinct per player), fresh task state."""
    d["tasks"][e] = (np.arange(P) + shift + e) % N_TASKS
    d["tstate"][e] = np.zeros(P, abi.task_state_dtype())


crowd, inventories, listings = _edit(_crowd), _edit(_inventories), _edit(_listings)
out_of_realm, task_swap = _edit(_out_of_realm), _edit(_task_swap)

# a whole 16-agent obs group, a whole 4-agent wave slice of another (agents 16 g + w + 4 j), singles
GROUP_OUT = tuple(range(16, 32)) + (49, 53, 57, 61) + (0, 77, 127)
SINGLES_OUT = (5, 40, 126)


def state(base, specs, P=128, S=384):
    """One schedule state: specs[e] = dict(crowd=k, inv=kind, listings=m, out=players, swap=bool)
    applied to env e of the reset blob `base`, in that order."""
    blob = base
    for e, sp in enumerate(specs):
        kw = dict(envs=(e,), P=P, S=S)
        blob = crowd(blob, sp["crowd"], **kw)
        if sp.get("inv"):
            blob = inventories(blob, sp["inv"], **kw)
        blob = listings(blob, sp["listings"], **kw)
        if sp.get("out"):
            blob = out_of_realm(blob, sp["out"], **kw)
        if sp.get("swap"):
            blob = task_swap(blob, **kw)
    return blob


def saturated(P=128):
    return dict(crowd=P, inv="full", listings=INV * P)


def _s(c, m, **kw):
    return dict(crowd=c, listings=m, **kw)


SAT, SAT_OUT = saturated(), dict(saturated(), out=GROUP_OUT)
# Env 0: listings 0 -> 1024 -> 257 -> 256 -> 25 -> 24 (-> repeated -> task swap) -> 0 -> 961 -> 960
# -> 1536 (-> full group out -> back) -> 1, crowd 128 -> 1 -> 101 -> 100 -> 99 -> 2.
ENV0 = [_s(128, 0, inv="mixed"), _s(1, 1024), _s(101, 257), _s(100, 256), _s(99, 25),
        _s(2, 24, inv="mixed", out=SINGLES_OUT), _s(2, 24, inv="mixed", out=SINGLES_OUT),
        _s(2, 24, inv="mixed", out=SINGLES_OUT, swap=True),
        _s(128, 0), _s(128, 961), _s(128, 960), SAT, SAT_OUT, SAT, _s(64, 1)]
# Env 1: the other listing counts (1023, 255, 89, 88) and the same thresholds at other steps
ENV1 = [_s(2, 1023), _s(99, 255), _s(100, 89), _s(101, 88), _s(1, 961),
        _s(99, 1, out=SINGLES_OUT), _s(99, 1, out=SINGLES_OUT), SAT, SAT_OUT, SAT,
        _s(128, 0, inv="mixed"), _s(128, 960), _s(1, 1024), _s(64, 257), _s(64, 25)]
REPEAT = (5, 6)       # schedule steps holding the same blob (both envs unchanged)
SWAP = (6, 7)         # env 0 differs only in its task assignment
SAT_STEPS = {0: (11, 12, 13), 1: (7, 8, 9)}  # per env: saturated, full group out, everyone back
assert len(ENV0) == len(ENV1) and all(a != b for a, b in zip(ENV0, ENV1))
assert ENV0[REPEAT[0]] == ENV0[REPEAT[1]] and ENV1[REPEAT[0]] == ENV1[REPEAT[1]]

_cache: dict = {}


def schedule():
    """[(name, blob)]: the fixed transition schedule at C4 size, built once per process."""
    if "s" not in _cache:
        base = reset_blob(config())
        out = []
        for i, specs in enumerate(zip(ENV0, ENV1)):
            if i == REPEAT[1]:
                out.append((f"{i}: repeat of {i - 1}", out[-1][1]))
                continue
            name = " | ".join(f"crowd {s['crowd']} listings {s['listings']}" + (" out" if s.get("out") else "")
                              + (" swap" if s.get("swap") else "") for s in specs)
            out.append((f"{i}: {name}", state(base, specs)))
        _cache["s"] = out
    return _cache["s"]


def saturated_pair(P: int, N: int, out):
    """(saturated, the same with `out` out of the realm) at another size, both envs."""
    base = reset_blob(config(P, N))
    S = P + N
    a = state(base, [saturated(P)] * N_ENVS, P, S)
    return a, out_of_realm(a, out, P=P, S=S)


# ---------------------------------------------------------------- numpy restatements (SPEC §8, §9)
def window_ids(d, e, P, S):
    """Per player: None when out of the realm, else (ids shown, entities in window): the ids of the
    entities in the realm within L-inf <= 7, ascending datastore row, cut to 100."""
    ent = d["ent"][e].astype(np.int64)
    alive = ent[F["alive"]] != 0
    slots = np.flatnonzero(alive)
    slots = slots[np.argsort(ent[F["ds_row"], slots], kind="stable")]
    r, c, ids = ent[F["row"], slots], ent[F["col"], slots], ent[F["id"], slots]
    out = []
    for p in range(P):
        if not alive[p]:
            out.append(None)
            continue
        near = np.maximum(np.abs(r - ent[F["row"], p]), np.abs(c - ent[F["col"], p])) <= 7
        out.append((ids[near][:100], int(near.sum())))
    return out


def priced_rows(d, e, P):
    """(rows, owners, prices) of the listed items in ascending item row, uncut."""
    it = d["items"][e].astype(np.int64)
    found = []
    for p in range(P):
        for k in range(_ninv(d["items"][e, p])):
            price = (it[p, k, 0] >> 10) & 127
            if price:
                found.append((it[p, k, 1] >> 16, p, price))
    found.sort()
    a = np.array(found, np.int64).reshape(-1, 3)
    return a[:, 0], a[:, 1], a[:, 2]


def buy_bits(d, e, P):
    """[P, 1025] Buy.MarketItem (SPEC §9): listing j < 1024 buyable iff price <= gold and not the
    agent's own; entry 1024 (no-op) set; rows of players out of the realm all zero."""
    _, own, price = priced_rows(d, e, P)
    own, price = own[:1024], price[:1024]
    gold = d["ent"][e, F["gold"], :P].astype(np.int64)
    out = np.zeros((P, 1025), np.float32)
    out[:, :own.size] = (price[None, :] <= gold[:, None]) & (own[None, :] != np.arange(P)[:, None])
    out[:, 1024] = 1
    out[d["ent"][e, F["alive"], :P] == 0] = 0
    return out


def counts(blob, P=128, S=384):
    """Per env: nv [P] (-1 out of the realm), in-window counts, ninv [P], priced items, table size."""
    d = split_state(blob, N_ENVS, S, P)
    out = []
    for e in range(N_ENVS):
        win = window_ids(d, e, P, S)
        nv = np.array([-1 if w is None else len(w[0]) for w in win])
        inw = np.array([0 if w is None else w[1] for w in win])
        ninv = np.array([_ninv(d["items"][e, p]) for p in range(P)])
        shown = set()
        for w in win:
            if w is not None:
                shown.update(w[0].tolist())
        out.append(dict(nv=nv, in_window=inw, ninv=ninv, priced=len(priced_rows(d, e, P)[0]), ne=len(shown)))
    return out


def wire_max_bytes(n: int, P: int) -> int:
    """nmmo_wire_max_bytes restated: full windows and inventories, a full table, every listing."""
    rec = owire.record_bytes(0x8000 | 100 | 12 << 7)
    return owire.header_bytes(n, P) + n * (owire.table_bytes(384) + P * rec + abi.NATIVE_MARKET_BYTES)


def wire_expect(blob, P=128, S=384):
    """(total bytes a wire buffer of this state announces, the largest record, listings per env),
    from the blob alone: header + per env its entity table, records and listings (SPEC §8c)."""
    total, rec_max, nms = owire.header_bytes(N_ENVS, P), 0, []
    for c in counts(blob, P, S):
        recs = [owire.record_bytes(0x8000 | int(v) | int(i) << 7) for v, i in zip(c["nv"], c["ninv"]) if v >= 0]
        nm = min(c["priced"], abi.MARKET_ROWS)
        total += owire.table_bytes(c["ne"]) + sum(recs) + 32 * nm
        rec_max = max([rec_max] + recs)
        nms.append(nm)
    return total, rec_max, nms
