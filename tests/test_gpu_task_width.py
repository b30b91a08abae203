"""The flat row at Task widths other than 2,048 on MI355X, bit-exact against the CPU oracle. The Task
width (TASK_EMBED_DIM) is the layout's one run-time value: it moves the Tile offset and the row
length, every other offset is a compile-time constant (csrc/obs_layout.h). 64 is below the 2,048
floats the full-write kernel prefetches per row, 2,112 above (its tail loop runs).

  P = 24, NPC = 40 (S = 64): the tracked handle runs flat_obs_kernel<., 0>, the NMMO_OBS_REZERO=1
    handle the full-write obs_kernel;
  P = 13, NPC = 6 (S = 19, not a multiple of 8): the tracked handle runs flat_obs_kernel<., 0, false>
    (the Entity columns staged element by element);
  at 2,112: a wire buffer decoded on store (wire_expand_kernel) and a record-stored batch decoded on
    gather (record_gather_kernel) against the flat rows of the same state."""

import numpy as np
import pytest
import torch

from nmmo_amd import abi
from oracle.oracle import OracleEnvs
from tests import obs_scenarios as sc
from tests.conftest import gpu_available
from tests.test_gpu_obs_saturation import _same

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

N = sc.N_ENVS
N_TASKS = 29  # > both player counts: a distinct task per player
STEPS = 4


def _set_tasks(handle, width, P):
    """TickGE tasks with distinct non-zero fp16 embeddings of the width under test."""
    from nmmo_amd import tasks as T

    rng = np.random.default_rng(width)
    emb = rng.uniform(0.25, 4.0, (N_TASKS, width)).astype(np.float16)
    emb[:, ::2] *= -1
    assert np.all(emb != 0) and len({e.tobytes() for e in emb}) == N_TASKS
    tl = [T.task("TickGE", num_tick=20 + i) for i in range(N_TASKS)]
    handle.set_tasks(tl, emb, np.tile(np.arange(P, dtype=np.int32) % N_TASKS, (N, 1)))


def _engine(width, P, NPC, lay=abi.OBS_FLAT):
    from nmmo_amd.engine import NmmoEngine

    eng = NmmoEngine(sc.config(P, NPC, obs_layout=lay, TASK_EMBED_DIM=width), N, seed=3)
    _set_tasks(eng, width, P)
    return eng


def _oracle(width, P, NPC):
    orc = OracleEnvs(sc.config(P, NPC, TASK_EMBED_DIM=width), N, seed=17)
    _set_tasks(orc, width, P)
    orc.reset()
    return orc


def _walk(width, P, NPC, engs):
    """Reset state, then STEPS scripted ticks: every handle's rows against the oracle's after each.
    Returns the oracle."""
    orc = _oracle(width, P, NPC)
    elems = 21264 + width + 225 * 3  # ActionTargets .. Market | Task | Tile
    assert orc.obs_elems == elems
    blob = orc.get_state()
    for name, h in engs.items():
        assert h.obs_elems == elems
        h.set_state(blob)
        h.observe()
        _same(h.obs, torch.from_numpy(orc.obs).to(h.device), f"{name} width {width} P {P}: reset")
    for t in range(STEPS):
        acts = orc.scripted_actions(40 + t)
        orc.step(acts)
        for name, h in engs.items():
            h.step(torch.from_numpy(acts).to(h.device))
            _same(h.obs, torch.from_numpy(orc.obs).to(h.device), f"{name} width {width} P {P}: tick {t}")
            assert h.get_fault() == 0
    task = torch.from_numpy(orc.obs[..., 21264:21264 + width])
    assert bool((task != 0).any()) and bool((torch.from_numpy(orc.obs[..., 21264 + width:]) != 0).any())
    return orc


@pytest.mark.parametrize("width", [64, 2112])
def test_flat_rows_at_task_width(width, monkeypatch):
    P, NPC = 24, 40
    tracked = _engine(width, P, NPC)
    monkeypatch.setenv("NMMO_OBS_REZERO", "1")
    rezero = _engine(width, P, NPC)
    monkeypatch.delenv("NMMO_OBS_REZERO")
    engs = {"tracked": tracked, "rezero": rezero}
    orc = _walk(width, P, NPC, engs)
    if width == 2112:  # the two record decoders, against the tracked handle's rows of the same state
        from nmmo_amd.storage import DeviceExperience

        wire = _engine(width, P, NPC, abi.OBS_WIRE)
        wire.set_state(orc.get_state())
        wire.observe()
        dev, elems = tracked.device, tracked.obs_elems
        xs = {k: DeviceExperience(N * P, elems, N * P, device=dev, record_arena_bytes=arena)
              for k, arena in (("flat", 0), ("wire", 0), ("records", 1 << 20))}
        z = torch.zeros(N * P, device=dev)
        acts = torch.zeros((N * P, 12), dtype=torch.int32, device=dev)
        m = torch.from_numpy(orc.mask.reshape(-1).astype(np.uint8)).to(dev)
        for k, x in xs.items():
            e = tracked if k == "flat" else wire
            x.store(e.obs, z, z.to(torch.uint8), m, acts, z, z, step=0, engine=None if k == "flat" else e)
        torch.cuda.synchronize()
        k = xs["flat"].ptr
        assert k > 0 and all((x.ptr, x.status) == (k, 0) for x in xs.values()), {n: (x.ptr, x.status) for n, x in xs.items()}
        want = xs["flat"].obs[:k]
        assert bool((want[:, 21264:] != 0).any())
        assert torch.equal(xs["wire"].obs[:k].view(torch.int32), want.view(torch.int32)), "decode on store"
        got = xs["records"].gather_obs(torch.arange(k, dtype=torch.int32, device=dev))
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "records"
        assert wire.get_fault() == 0
        wire.close()
    for h in engs.values():
        h.close()


@pytest.mark.parametrize("width", [64, 2112])
def test_flat_rows_at_task_width_odd_slots(width):
    eng = _engine(width, 13, 6)
    _walk(width, 13, 6, {"tracked": eng})
    eng.close()
