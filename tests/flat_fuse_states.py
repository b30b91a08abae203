"""The states tests/test_gpu_flat_fuse.py steps from to cross flat_obs.hip's gather threshold
(kFoGather = 12 visible rows per agent come from LDS, the rest from the mirror in HBM) and the
100-row Entity cut, built with tests/obs_scenarios.py's builders. tests/test_flat_fuse_states.py
shows on the CPU oracle that one scripted step from them reaches the counts claimed. A plain module
the two tests import, not a conftest."""

from __future__ import annotations

import numpy as np

from nmmo_amd import abi
from oracle.oracle import split_state
from tests import obs_scenarios as sc

K_GATHER = 12      # flat_obs.hip kFoGather
ACTION_SEED = 900  # the one scripted step taken from every state
# (env 0's crowd, env 1's crowd) per state, walked in this order over the same obs buffer: an env's
# counts rise and fall across the gather threshold and the 100-row cut from state to state
CROWDS = [(128, 16), (2, 20), (101, 14), (13, 128), (100, 18)]
# in-window counts some agent must have after the step
NEED = (K_GATHER - 1, K_GATHER, K_GATHER + 1, 99, 100, 101)

_cache: dict = {}


def _high_rows(d, e, P, S):
    """Every third entity in the realm (players and NPCs) moves to a free datastore row in 257..384
    (a reset env uses rows 1..145 only): its old row takes that row's place on the free ring. The
    window order (ascending datastore row) then interleaves slots differently too."""
    ent, env, ring = d["ent"][e], d["env"][e], d["ring"][e]
    free = [(int(env[sc.E["free_head"]]) + i) % S for i in range(int(env[sc.E["free_count"]]))]
    free = [i for i in free if ring[i] >= 257]
    movers = [s for s in range(S) if ent[sc.F["alive"], s]][e::3]
    assert len(free) >= len(movers) > 40
    for s, i in zip(movers, free):
        ent[sc.F["ds_row"], s], ring[i] = ring[i], ent[sc.F["ds_row"], s]


high_rows = sc._edit(_high_rows)


def states():
    """[(name, blob)] at C4 size, built once per process."""
    if "s" not in _cache:
        base = high_rows(sc.reset_blob(sc.config()))
        _cache["s"] = [(f"crowds {a} | {b}", sc.state(base, [sc._s(a, 0, inv="mixed"), sc._s(b, 5, inv="mixed")]))
                       for a, b in CROWDS]
    return _cache["s"]


def high_rows_seen(blob, P=128, S=384) -> int:
    """Entities on datastore rows 257..384 that some player in the realm shows among its first 100."""
    d = split_state(blob, sc.N_ENVS, S, P)
    n = 0
    for e in range(sc.N_ENVS):
        ent = d["ent"][e].astype(np.int64)
        by_id = {int(ent[abi.F["id"], s]): int(ent[abi.F["ds_row"], s]) for s in range(S) if ent[abi.F["alive"], s]}
        for w in sc.window_ids(d, e, P, S):
            if w is not None:
                n += sum(1 for i in w[0].tolist() if by_id[i] >= 257)
    return n
