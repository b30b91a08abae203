"""The states tests/test_gpu_flat_maskpass.py steps from: the smallest cases at which the mask pass of
flat_obs.hip's mirror variant (the tracked ActionTargets chunks of a wave's four agents
built once, lane = (agent, chunk)) can go wrong, built with tests/obs_scenarios.py's builders. A wave
of the kernel writes agents 16 g + w + 4 j (j = 0..3) of one env. tests/test_flat_maskpass_states.py
shows on the CPU oracle that one no-op step from each state leaves the counts claimed here. A plain
module the two tests import, not a conftest.

Every step of the walk takes no-op actions (players stay where the state put them; the NPCs near the
clusters are moved away first), so what a state sets up is what the obs launch of the step sees."""

from __future__ import annotations

import numpy as np

from nmmo_amd import abi, layout
from oracle.oracle import split_state
from tests import obs_scenarios as sc

K_ROWS = 16  # flat_obs.hip kFoPassRows: the visible rows a lane group of the mask pass covers
F, INV = abi.F, abi.INV_SLOTS
HEAD = layout.HEAD
# every head's no-op (last) index, price heads and the style 0 (SPEC §10)
NOOP = np.array([0 if k in (HEAD["Attack.Style"], HEAD["GiveGold.Price"], HEAD["Sell.Price"]) else n - 1
                 for k, n in enumerate(layout.ACTION_DIMS)], np.int32)
PRICES = (0, 63, 64, 98)  # the wrapper's last price of agent p: PRICES[(p // 4) % 4], wave mates differ
GOLD_EDGES = {16: 0, 20: 1, 24: 98, 28: 99, 17: 100, 21: 0, 25: 99, 29: 1}  # agent -> gold (waves 0 and 1 of group 1)
LISTING_COUNTS = (0, 1, 24, 25, 63, 64, 65, 959, 960, 961)
CROWD = 12  # listing_states: with the NPCs beside the block the counts straddle K_ROWS

# clusters of env 0: (observer, members in datastore-row order); every member stands within two tiles
# of the observer, the last two (odd ids: past their spawn immunity) on the observer's own tile. The
# observers 0, 4, 8 and the loner 12 are wave 0 of group 0: K_ROWS - 1, K_ROWS, K_ROWS + 1 and 1 rows.
CLUSTERS = [
    (0, [0] + list(range(32, 44)) + [117, 119]),
    (4, [4] + list(range(44, 57)) + [121, 123]),
    (8, [8] + list(range(57, 71)) + [125, 127]),
]
LONERS = (12, 1, 5)
assert [len(m) for _, m in CLUSTERS] == [K_ROWS - 1, K_ROWS, K_ROWS + 1]
# env 1: a block of BIG players around observer 0 (each sees more than 100), observers 4, 8, 12 alone
BIG = 104
BIG_LONERS = (4, 8, 12)
R0, C0, STEP = 34, 30, 18  # spots (R0 + STEP i, C0 + STEP j): more than two windows apart

_cache: dict = {}


def noop_actions(prices=False, P=128) -> np.ndarray:
    a = np.tile(NOOP, (sc.N_ENVS, P, 1))
    if prices:
        a[:, :, HEAD["Sell.Price"]] = np.array([PRICES[(p // 4) % 4] for p in range(P)], np.int32)[None, :]
    return a


def _spot(i):
    return R0 + STEP * (i // 5), C0 + STEP * (i % 5)


def _clear(ent, keep, S):
    """Every entity that is not in `keep` leaves the spots' region (40 rows down: still in the map)."""
    lo_r, hi_r, lo_c, hi_c = R0 - 12, R0 + STEP + 12, C0 - 12, C0 + 4 * STEP + 12
    for s in range(S):
        if s not in keep and lo_r <= ent[F["row"], s] <= hi_r and lo_c <= ent[F["col"], s] <= hi_c:
            ent[F["row"], s] += 40
            assert ent[F["row"], s] < 143 - 8


def _clusters(d, e, P, S):
    ent = d["ent"][e]
    ring = [(dr, dc) for dr in range(-2, 3) for dc in range(-2, 3) if (dr, dc) != (0, 0)]
    if e == 0:
        keep = {m for _, ms in CLUSTERS for m in ms} | set(LONERS)
        _clear(ent, keep, S)
        for i, (_, ms) in enumerate(CLUSTERS):
            r, c = _spot(i)
            for k, m in enumerate(ms):
                dr, dc = (0, 0) if k == 0 or k >= len(ms) - 2 else ring[k - 1]
                ent[F["row"], m], ent[F["col"], m] = r + dr, c + dc
        for i, p in enumerate(LONERS):
            ent[F["row"], p], ent[F["col"], p] = _spot(len(CLUSTERS) + i)
    else:
        big = [0] + [p for p in range(13, P)][:BIG - 1]
        keep = set(big) | set(BIG_LONERS)
        _clear(ent, keep, S)
        r, c = _spot(0)
        for k, m in enumerate(big):  # an 8 x 8 block, two per tile: everyone within 7 of everyone
            ent[F["row"], m], ent[F["col"], m] = r - 3 + (k // 2) // 8, c - 3 + (k // 2) % 8
        ent[F["row"], big[-1]], ent[F["col"], big[-1]] = ent[F["row"], 0], ent[F["col"], 0]
        for i, p in enumerate(BIG_LONERS):
            ent[F["row"], p], ent[F["col"], p] = _spot(2 + i)


def _gold(d, e, P, S):
    for p, g in GOLD_EDGES.items():
        d["ent"][e, F["gold"], p] = g


def _edge_owners(d, e, P, S):
    """The owners of the listings at the edges of Buy's words (listing 0, 63 or the last, the last) can
    afford them: their Buy entry is clear because the listing is their own."""
    _, own, _ = sc.priced_rows(d, e, P)
    m = min(len(own), abi.MARKET_ROWS)
    for k in ({0, min(m, 64) - 1, m - 1} if m else ()):
        d["ent"][e, F["gold"], int(own[k])] = 95


def _npcs_back(d, e, P, S):
    """The NPCs crowd() put in the row above the block, five rows further up: still in every window of
    the crowd's row, out of attack range for the two steps a state is stepped (one of them kills a
    player with one hit, and its listings go with it)."""
    ent = d["ent"][e]
    r0 = int(ent[F["row"], 0]) - 1
    for s in range(P, S):
        if ent[F["alive"], s] and ent[F["row"], s] == r0:
            ent[F["row"], s] -= 5


def _dangerous(d, e, P, S):
    """The NPCs crowd() put beside the block: every other one dangerous (npc_type 3)."""
    ent = d["ent"][e]
    r0 = int(ent[F["row"], 0]) - 1 - 5  # (after npcs_back: brought back beside the block)
    near = [s for s in range(P, S) if ent[F["alive"], s] and ent[F["row"], s] == r0]
    assert near
    for s in near:
        ent[F["row"], s] += 5
    for s in near[::2]:
        ent[F["npc_type"], s] = 3


clusters, gold, dangerous = sc._edit(_clusters), sc._edit(_gold), sc._edit(_dangerous)
edge_owners, npcs_back = sc._edit(_edge_owners), sc._edit(_npcs_back)


def base():
    if "b" not in _cache:
        _cache["b"] = sc.reset_blob(sc.config())
    return _cache["b"]


def group_states():
    """[(name, blob)]: the lane-group bound (env 0: 15 / 16 / 17 / 1 rows in one wave; env 1: more than
    100 rows beside agents that see 1), with mixed inventories (0, 1, 11, 12 items), a few listings
    and the gold edges."""
    if "g" not in _cache:
        b = sc.state(base(), [sc._s(1, 25, inv="mixed"), sc._s(1, 64, inv="mixed")])
        _cache["g"] = [("lane groups", gold(clusters(b)))]
    return _cache["g"]


def listing_states():
    """[(name, blob)]: the listing counts, two per state (env 0, env 1), a crowd of CROWD players and its NPCs
    (agents of one wave see more rows than a lane group holds and fewer), mixed inventories, the gold edges."""
    if "l" not in _cache:
        out = []
        for a, b in zip(LISTING_COUNTS[::2], LISTING_COUNTS[1::2]):
            blob = npcs_back(sc.state(base(), [sc._s(CROWD, a, inv="mixed"), sc._s(CROWD, b, inv="mixed")]))
            out.append((f"listings {a} | {b}", edge_owners(gold(blob))))
        _cache["l"] = out
    return _cache["l"]


def danger_state():
    """(name, blob): listings 24 | 25 with every other NPC beside the crowd dangerous (npc_type 3),
    for the wrappers' no-dangerous-NPC edit."""
    if "d" not in _cache:
        name, blob = listing_states()[1]
        _cache["d"] = (name + ", dangerous NPCs", dangerous(blob))
    return _cache["d"]


def mixed_states():
    """(everyone in, a wave slice / a group / singles out): stepping from one to the other over the
    same buffer gives rows in the realm, dead for several ticks, dead since this tick and back this
    tick, in the same waves."""
    if "m" not in _cache:
        a = listing_states()[1][1]  # listings 24 | 25
        _cache["m"] = (a, sc.out_of_realm(a, sc.GROUP_OUT))
    return _cache["m"]


def post_counts(orc, blob, actions):
    """sc.counts of the state one step after `blob`, and that state."""
    orc.set_state(blob)
    orc.step(actions)
    post = orc.get_state()
    return sc.counts(post), post


def wave_of(p):
    return p // 16, p % 4


def same_tile_attackable(post, e, p, k, P=128, S=384):
    """Visible row k of player p (env e) is another player on p's tile, past its spawn immunity."""
    d = split_state(post, sc.N_ENVS, S, P)
    ent = d["ent"][e].astype(np.int64)
    slots = np.flatnonzero(ent[F["alive"]] != 0)
    slots = slots[np.argsort(ent[F["ds_row"], slots], kind="stable")]
    near = np.maximum(np.abs(ent[F["row"], slots] - ent[F["row"], p]), np.abs(ent[F["col"], slots] - ent[F["col"], p])) <= 7
    vis = slots[near]
    if k >= len(vis):
        return False
    s = int(vis[k])
    return (s < P and s != p and ent[F["row"], s] == ent[F["row"], p] and ent[F["col"], s] == ent[F["col"], p]
            and ent[F["time_alive"], s] >= 20)
