"""The flat rows' tick-fused entity mirror on MI355X: a step whose obs launch goes
to flat_obs_kernel at 384 slots / 128 players has its tick write the packed datastore-row words and
a slot-major copy of the Entity columns (tick.hip flat_mirror_fused), and the obs launch reads those
instead of staging the env's columns. NMMO_FLAT_FUSE=0 at create keeps the staging path: the two
must write the same bytes, and the mirror must never be read by a launch other than the one of the
step that wrote it.

  1. fused == staged tick by tick (obs bytes, step outputs, obs counter, final state), plain, with
     the start-kit wrapper (the kWrap variant) and with the Tile sections invalidated every step;
  2. the gather threshold (kFoGather visible rows from LDS, the rest from HBM), the 100-row cut and
     datastore rows 257..384 against the oracle (tests/flat_fuse_states.py; the counts are asserted
     on the CPU by tests/test_flat_fuse_states.py);
  3. a stale mirror is never read: set_state / observe, step(write_obs=False) + observe, step_envs
     on a subset, reset mid-run;
  4. a captured graph of 3 steps replayed equals eager steps."""

import numpy as np
import pytest
import torch

from nmmo_amd import abi
from tests import flat_fuse_states as fs
from tests import obs_scenarios as sc
from tests.conftest import gpu_available
from tests.test_gpu_obs_saturation import _oracle_rows, _same

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

N = 4  # envs of the fused-vs-staged runs: 32 obs workgroups, 4 tick workgroups


def _pair(monkeypatch, n=N, seed=11, early_stop=8, wrapper=None):
    """(fused, staged): same config and seed, the second created under NMMO_FLAT_FUSE=0."""
    from nmmo_amd.config import Config
    from nmmo_amd.engine import NmmoEngine
    from nmmo_amd.wrappers import wrapper_config

    cfg = Config.preset("C4", MAP_N=4, early_stop_agent_num=early_stop)
    monkeypatch.delenv("NMMO_FLAT_FUSE", raising=False)
    a = NmmoEngine(cfg, n, seed=seed)
    monkeypatch.setenv("NMMO_FLAT_FUSE", "0")
    b = NmmoEngine(cfg, n, seed=seed)
    monkeypatch.delenv("NMMO_FLAT_FUSE")
    for e in (a, b):
        if wrapper:
            e.set_wrapper(wrapper_config(wrapper, heal_bonus_weight=0.03, explore_bonus_weight=0.01))
    return a, b


def _equal(a, b, what):
    assert torch.equal(a.obs.view(torch.int32), b.obs.view(torch.int32)), f"{what}: obs bytes differ"
    for k in ("rew", "term", "trunc", "mask"):
        x, y = getattr(a, k), getattr(b, k)
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y), f"{what}: {k} differs"


@pytest.mark.parametrize("mode", ["plain", "wrapper", "tile-invalidate"])
def test_fused_equals_staged_tick_by_tick(mode, monkeypatch):
    a, b = _pair(monkeypatch, wrapper="neurips23_start_kit" if mode == "wrapper" else None)
    ca, cb = (torch.zeros((N, 2), dtype=torch.int64, device=a.device) for _ in range(2))
    a.set_obs_counter(ca)
    b.set_obs_counter(cb)
    a.reset()
    b.reset()
    _equal(a, b, "reset")
    left = torch.zeros((), dtype=torch.bool, device=a.device)
    for t in range(200):
        if t in (40, 41, 90, 150):  # forced episode ends: in-kernel resets between culls
            m = np.arange(N) % 2 == t % 2
            a.end_episodes(m)
            b.end_episodes(m)
        for e in (a, b):
            e.scripted_actions(1000 + t)
            if mode == "tile-invalidate":
                e.obs_invalidate_sections(abi.OBS_SEC_TILE)
            e.step()
        _equal(a, b, f"tick {t}")
        assert torch.equal(ca, cb), f"tick {t}: obs counter {ca.tolist()} != {cb.tolist()}"
        left |= (a.mask.sum(1) < a.P).any()
    assert bool(left), "no agent left the realm"
    assert int(ca[:, 1].sum().item()) > 0
    assert np.array_equal(a.get_state(), b.get_state())
    assert a.get_fault() == 0 and b.get_fault() == 0
    a.close()
    b.close()


def test_gather_threshold_walk_against_the_oracle():
    from nmmo_amd.engine import NmmoEngine

    eng = NmmoEngine(sc.config(obs_layout=abi.OBS_FLAT), sc.N_ENVS, seed=3)
    sc.set_tasks(eng, 128)
    orc = sc.make_oracle(sc.config())
    errs = []
    for name, blob in fs.states():  # one after another over the same buffer
        orc.set_state(blob)
        eng.set_state(blob)
        acts = orc.scripted_actions(fs.ACTION_SEED)
        orc.step(acts)
        eng.step(torch.from_numpy(acts).to(eng.device))
        torch.cuda.synchronize()
        assert np.array_equal(eng.get_state(), orc.get_state()), name
        _same(eng.obs, torch.from_numpy(orc.obs).to(eng.device), f"{name}: fused step vs oracle", errs)
    assert not errs, "\n".join(errs)
    assert eng.get_fault() == 0
    eng.close()


def test_stale_mirror_is_never_read():
    """The mirror holds the state of the last fused step; set_state changes the state behind it."""
    from nmmo_amd.engine import NmmoEngine

    eng = NmmoEngine(sc.config(obs_layout=abi.OBS_FLAT), sc.N_ENVS, seed=3)
    sc.set_tasks(eng, 128)
    orc = sc.make_oracle(sc.config())
    (_, s0), (_, s1) = fs.states()[0], fs.states()[1]
    for h in (eng, orc):
        h.set_state(s0)
    acts = orc.scripted_actions(fs.ACTION_SEED)
    orc.step(acts)
    eng.step(torch.from_numpy(acts).to(eng.device))  # fused: the mirror holds s0's successor
    for h in (eng, orc):
        h.set_state(s1)
    eng.observe()
    _same(eng.obs, _oracle_rows(orc, eng.device), "observe after set_state")
    acts = orc.scripted_actions(fs.ACTION_SEED + 1)
    orc.step(acts)
    eng.step(torch.from_numpy(acts).to(eng.device))
    _same(eng.obs, torch.from_numpy(orc.obs).to(eng.device), "step after set_state")
    assert eng.get_fault() == 0
    eng.close()


def test_other_obs_paths_equal_the_staged_handle(monkeypatch):
    a, b = _pair(monkeypatch)
    ids = torch.tensor([2, 0], dtype=torch.int32, device=a.device)
    a.reset()
    b.reset()
    for t in range(24):
        for e in (a, b):
            e.scripted_actions(500 + t)
            if t % 6 == 2:  # the tick alone, then the gather: the mirror of an older step is stale
                e.step(write_obs=False)
                e.observe()
            elif t % 6 == 4:  # a subset (its tick and obs launch share the list), then everyone
                e.step_envs(ids)
            elif t == 13:
                e.reset()
            else:
                e.step()
        _equal(a, b, f"tick {t}")
    assert np.array_equal(a.get_state(), b.get_state())
    assert a.get_fault() == 0 and b.get_fault() == 0
    a.close()
    b.close()


def test_graph_of_three_steps_equals_eager(monkeypatch):
    from nmmo_amd.config import Config
    from nmmo_amd.engine import NmmoEngine

    cfg = Config.preset("C4", MAP_N=4, early_stop_agent_num=8)
    monkeypatch.delenv("NMMO_FLAT_FUSE", raising=False)
    a, b = NmmoEngine(cfg, N, seed=5), NmmoEngine(cfg, N, seed=5)

    def steps(e, k):
        for _ in range(k):
            e.scripted_actions(77)
            e.step()

    for e in (a, b):
        e.reset()
        steps(e, 2)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=a.device)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        steps(a, 3)
    for r in range(3):
        with torch.cuda.stream(s):
            g.replay()
        steps(b, 3)
        torch.cuda.synchronize()
        _equal(a, b, f"replay {r}")
    assert np.array_equal(a.get_state(), b.get_state())
    assert a.get_fault() == 0 and b.get_fault() == 0
    a.close()
    b.close()
