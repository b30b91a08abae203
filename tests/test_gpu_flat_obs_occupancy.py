"""flat_obs_kernel's LDS layout at five workgroups per CU: states aimed at the
regions that share or changed storage, bit-exact against the CPU oracle for a tracked handle and
a full-write (NMMO_OBS_REZERO=1) handle, every state written over the previous state's rows.

 - window rows staged realigned at 16 B: agents at columns of every residue mod 4, at the clamp
   edges (7 and 152, rows and columns), out of the realm at and beyond the edges, over a map of
   random materials (the reset map's border is one material: a misaligned row would not show);
 - 100 visible-row words per wave: windows holding 99, 100, 101 and more than 128 entities;
 - the listings' pool (price | owner entries from its start, item words from its end: every
   listing's item word up to 256 listings, 64 of them at 1,024): 63, 64, 65, 255, 256, 257 and
   1,024 listings (INV * P = 288 at the small shape), rising and falling across 256;
 - the packed datastore rows aliased onto the window rows' region: entities on datastore rows
   257..384 (the last two of a lane's six words) inside a window that shows them;
 - the item words kept in T's row / column columns: Entity rows' row / column entries, the
   Inventory section and the inventory-driven masks at every state.
Shapes: P = 128, NPC = 256 (the kS = 384 kernel) and P = 24, NPC = 40 (S = 64: the generic kernel,
item words after the window rows, a partial last agent group of 8).
`test_states_reach_their_counts` shows on the CPU that the states hold what is claimed."""

import numpy as np
import pytest

from nmmo_amd import abi
from oracle.oracle import join_state, split_state
from tests import obs_scenarios as sc
from tests.conftest import gpu_available

N, F, E = sc.N_ENVS, abi.F, abi.E
K, KMIN = 256, 64  # flat_obs.hip fo_staged: every listing's item word staged up to K, KMIN at 1,024
LO, HI = 7, 152  # ao_clamp_pos: kVision, kSize - 1 - kVision
# (agent, row, col): both clamp edges in rows and columns, every column residue mod 4 at each
EDGES = ((0, LO, LO), (1, LO, LO + 1), (2, 30, LO + 2), (3, 30, LO + 3), (4, HI, HI - 3), (5, HI, HI - 2),
         (6, 60, HI - 1), (7, 60, HI), (8, LO, HI), (9, HI, LO))
BEYOND = ((17, 2, 158), (18, 159, 0))  # out of the realm, outside the clamp range
SHAPES = {"c4": (128, 256), "small": (24, 40)}
OUT = {"c4": (5, 17, 18, 40, 126), "small": (5, 17, 18, 23)}
HIGH_ROWS = (257, 258, 319, 320, 321, 383, 384)  # word 4's first rows, the 4 | 5 boundary, the last row


def _edit(blob, P, S, fn):
    d = split_state(blob, N, S, P)
    fn(d)
    return join_state(d)


def _random_map(d, e, seed):
    d["mat"][e] = np.random.default_rng(seed).integers(0, 16, size=d["mat"][e].shape, dtype=d["mat"].dtype)


def _edges(d, e):
    for a, r, c in EDGES + BEYOND:
        d["ent"][e, F["row"], a], d["ent"][e, F["col"], a] = r, c


def _high_rows(d, e, slots):
    """Datastore rows HIGH_ROWS for `slots`, each swapped with the free-ring entry holding it."""
    env, ring, ent = d["env"][e], d["ring"][e], d["ent"][e]
    S = ring.shape[0]
    head, cnt = int(env[E["free_head"]]), int(env[E["free_count"]])
    live = (head + np.arange(cnt)) % S
    for s, row in zip(slots, HIGH_ROWS):
        assert ent[F["alive"], s]
        i = live[np.flatnonzero(ring[live] == row)]
        assert i.size == 1, f"datastore row {row} is not free"
        ring[i[0]], ent[F["ds_row"], s] = ent[F["ds_row"], s], row


_cache: dict = {}


def states(shape):
    """[(name, blob)] for SHAPES[shape], built once per process."""
    if shape in _cache:
        return _cache[shape]
    P, NPC = SHAPES[shape]
    S = P + NPC
    base = sc.reset_blob(sc.config(P, NPC))
    big = min(1024, abi.INV_SLOTS * P)

    def st(s0, s1):
        return sc.state(base, [s0, s1], P, S)

    def edge_state(m):  # env 0: m listings among the agents still in the realm
        blob = st(dict(crowd=1, listings=0), dict(crowd=min(99, P), listings=0))
        blob = _edit(blob, P, S, lambda d: (_edges(d, 0), _random_map(d, 0, 11), _random_map(d, 1, 12)))
        blob = sc.out_of_realm(blob, OUT[shape], envs=(0,), P=P, S=S)
        return sc.listings(blob, m, envs=(0,), P=P, S=S)

    if shape == "c4":
        hi = st(dict(crowd=64, listings=KMIN), dict(crowd=2, listings=K - 1))
        hi = _edit(hi, P, S, lambda d: _high_rows(d, 0, (1, 2, 3, 4, 5, 6, 7)))
        out = [("crowd 99 / 100, listings 63 / 256", st(dict(crowd=99, listings=KMIN - 1), dict(crowd=100, listings=K))),
               ("crowd 101 / 128, listings 65 / 1024", st(dict(crowd=101, listings=KMIN + 1), dict(crowd=128, listings=big))),
               ("datastore rows 257..384, listings 64 | 1024 -> 255", hi),
               ("edges, random map, out of the realm, listings 257 / 0", edge_state(K + 1)),
               ("crowd 128 / 101, listings 256 / 1024", st(dict(crowd=128, listings=K), dict(crowd=101, listings=big)))]
    else:
        out = [("listings 63 / 64", st(dict(crowd=P, listings=KMIN - 1), dict(crowd=13, listings=KMIN))),
               ("listings 257 / INV * P", st(dict(crowd=P, listings=K + 1), dict(crowd=P, listings=big))),
               ("edges, random map, out of the realm, listings 65 / 0", edge_state(KMIN + 1)),
               ("listings 256 / 255", st(dict(crowd=1, listings=K), dict(crowd=P, listings=K - 1)))]
    _cache[shape] = out
    return out


def test_states_reach_their_counts():
    cs = {sh: [sc.counts(b, SHAPES[sh][0], sum(SHAPES[sh])) for _, b in states(sh)] for sh in SHAPES}
    inw = {int(v) for c in cs["c4"] for e in range(N) for v in c[e]["in_window"]}
    assert {99, 100, 101} <= inw and max(inw) > 128, sorted(inw)
    counts = {KMIN - 1, KMIN, KMIN + 1, K - 1, K, K + 1}
    assert counts | {1024} <= {c[e]["priced"] for c in cs["c4"] for e in range(N)}
    assert counts | {abi.INV_SLOTS * 24} <= {c[e]["priced"] for c in cs["small"] for e in range(N)}
    for e in range(N):  # the staged / fallback threshold is crossed in both directions
        nm = [c[e]["priced"] for c in cs["c4"]]
        assert any(a > K >= b for a, b in zip(nm, nm[1:])) and any(a <= K < b for a, b in zip(nm, nm[1:])), nm
    # the high datastore rows are shown: agent 0's window holds all of them below the 100-row cut
    P, S = 128, 384
    d = split_state(states("c4")[2][1], N, S, P)
    ent = d["ent"][0].astype(np.int64)
    near = (ent[F["alive"]] != 0) & (np.maximum(np.abs(ent[F["row"]] - ent[F["row"], 0]),
                                                np.abs(ent[F["col"]] - ent[F["col"], 0])) <= 7)
    assert near.sum() <= 100 and set(HIGH_ROWS) <= set(ent[F["ds_row"]][near].tolist())
    assert sorted(ent[F["ds_row"]][ent[F["alive"]] != 0].tolist() +
                  d["ring"][0][(int(d["env"][0, E["free_head"]]) + np.arange(int(d["env"][0, E["free_count"]]))) % S].tolist()
                  ) == list(range(1, S + 1)), "datastore rows and the free ring"
    for sh, (P, NPC) in SHAPES.items():  # the edge state: residues, both edges, agents gone at and beyond them
        d = split_state(states(sh)[-2][1], N, P + NPC, P)
        ent = d["ent"][0]
        live = [a for a, _, _ in EDGES if ent[F["alive"], a]]
        assert {int(ent[F["col"], a]) % 4 for a in live} == {0, 1, 2, 3}
        assert {LO, HI} <= {int(ent[F["col"], a]) for a in live} and {LO, HI} <= {int(ent[F["row"], a]) for a in live}
        assert not ent[F["alive"], 5] and not ent[F["alive"], 17] and not ent[F["alive"], 18]
        assert len(np.unique(d["mat"][0])) == 16
    assert SHAPES["small"][0] % 16 != 0 and sum(SHAPES["small"]) % 8 == 0


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs a GPU")
def test_walk_tracked_and_full_write_vs_oracle(shape, monkeypatch):
    from tests.test_gpu_obs_saturation import _flat_pair, _oracle_rows, _same

    P, NPC = SHAPES[shape]
    flat, rez = _flat_pair(monkeypatch, P, NPC)
    orc = sc.make_oracle(sc.config(P, NPC))
    errs = []
    for name, blob in states(shape):
        orc.set_state(blob)
        want = _oracle_rows(orc, flat.device)
        for what, h in (("tracked", flat), ("full write", rez)):
            h.set_state(blob)
            h.observe()
            _same(h.obs, want, f"{shape} {name}: {what} vs oracle", errs)
            assert h.get_fault() == 0, name
    assert not errs, "\n".join(errs)
    flat.close()
    rez.close()
