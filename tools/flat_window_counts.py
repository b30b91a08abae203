"""Distribution of the in-window entity count per agent row in the bench scenario (CPU; oracle-driven).

flat_obs.hip's mirror variant gathers the first kFoGather visible entities' mirror rows into LDS
ahead of the agent loop; the rows past them take a global load each. This replays
the bench's scenario on the oracle as tools/tick_lines.py does (staggered episode phases,
masked-uniform scripted actions) and prints, per agent in the realm and tick, the distribution of
the number of entities in its 15 x 15 window (itself included, capped at 100 as the obs rows are).

  python tools/flat_window_counts.py [C4] [envs] [stagger] [ticks]
"""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nmmo_amd import abi  # noqa: E402
from nmmo_amd.config import Config  # noqa: E402
from oracle.oracle import OracleEnvs, split_state  # noqa: E402

VISION = 7
N_OBS = 100


def window_counts(ent, players):
    """In-window counts of one env's players in the realm."""
    alive = ent[abi.F["alive"]] != 0
    r = ent[abi.F["row"]].astype(np.int64)
    c = ent[abi.F["col"]].astype(np.int64)
    pa = np.flatnonzero(alive[:players])
    d = np.maximum(np.abs(r[pa, None] - r[None, alive]), np.abs(c[pa, None] - c[None, alive]))
    return np.minimum((d <= VISION).sum(axis=1), N_OBS)


def main():
    preset = sys.argv[1] if len(sys.argv) > 1 else "C4"
    envs = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    stagger = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    ticks = int(sys.argv[4]) if len(sys.argv) > 4 else 64
    cfg = Config.preset(preset, early_stop_agent_num=8, obs_layout=abi.OBS_NONE)
    o = OracleEnvs(cfg, envs, seed=1)
    o.reset()
    for k in range(stagger):  # bench.py's staggered pre-roll
        o.end_episodes(np.arange(envs) % stagger == k)
        o.step(o.scripted_actions(1_000_003))
    n = []
    for t in range(ticks):
        st = split_state(o.get_state(), envs, o.S)
        n += [window_counts(st["ent"][e], o.P) for e in range(envs)]
        o.step(o.scripted_actions(1000 + t))
    n = np.concatenate(n)
    hist = np.bincount(n, minlength=N_OBS + 1)
    cum = np.cumsum(hist) / n.size
    print(f"{preset}: {envs} envs x {ticks} ticks, {n.size} agent rows: mean {n.mean():.2f} max {n.max()}")
    for k in range(1, int(n.max()) + 1):
        print(f"  {k:3d}: {hist[k]:8d}  cum {100 * cum[k]:7.3f} %")
    even = [k for k in range(2, N_OBS + 1, 2) if cum[k] >= 0.99]
    print(f"smallest even count covering >= 99 % of agent rows: {even[0]}")


if __name__ == "__main__":
    main()
