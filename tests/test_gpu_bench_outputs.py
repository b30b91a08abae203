"""bench.py's plain run and --dump-outputs on a small workload: --steps sets the timed steps, the
line carries ms_per_step, what --full measures is null without it, and two runs with the same
arguments write the same arrays."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS, P, STEPS = 6, 128, 13  # 13 = one 10-tick hipGraph + a 3-tick one


def _bench(out_dir, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C4",
                          "--envs", str(ENVS), "--steps", str(STEPS), "--warmup", "2", "--stagger", "3",
                          "--dump-outputs", str(out_dir), *extra],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    a, b = tmp_path_factory.mktemp("dump_a"), tmp_path_factory.mktemp("dump_b")
    return _bench(a), a, _bench(b), b


def test_plain_line(runs):
    d = runs[0]
    assert d["steps"] == STEPS and d["ms_per_step"] > 0 and d["unit"] == "agent-steps/s"
    assert d["higher_is_better"] is True and d["dtype"] == "int16"
    # the slot count of exactly STEPS timed steps (1% for ms_per_step's rounding)
    assert d["slot_steps_per_sec"] * d["ms_per_step"] / 1e3 == pytest.approx(ENVS * P, rel=0.01)
    assert 0 < d["value"] <= d["slot_steps_per_sec"]
    for k in ("kernel_ms", "roofline", "cpu_baseline", "extra_configs"):
        assert d[k] is None


def test_dumped_outputs(runs):
    _, a, _, b = runs
    names = sorted(f for f in os.listdir(a))
    assert names == ["mask.npy", "obs_sample.npy", "reward.npy", "terminated.npy", "truncated.npy"]
    assert sum(os.path.getsize(os.path.join(a, f)) for f in names) <= 64 << 20
    for f in names:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert x.dtype == np.float32 and np.array_equal(x, y), f
    mask, obs = np.load(os.path.join(a, "mask.npy")), np.load(os.path.join(a, "obs_sample.npy"))
    assert mask.shape == (ENVS, P) and set(np.unique(mask)) <= {0.0, 1.0} and mask.sum() > 0
    assert obs.shape == (min(ENVS * P, (40 << 20) // (4 * 23987)), 23987) and np.abs(obs).sum() > 0
