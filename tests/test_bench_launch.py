"""bench.py's multi-rank launcher (CPU only, no GPU call): `--gpus N` without WORLD_SIZE starts
N ranks under torch.distributed.run with RANK/WORLD_SIZE set; under torchrun a WORLD_SIZE that
differs from --gpus is refused."""

import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(kw)
    return env


def test_gpus_n_spawns_n_ranks():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-launch"],
                         capture_output=True, text=True, timeout=180, env=_env())
    assert out.returncode == 0, out.stderr
    lines = [json.loads(s) for s in out.stdout.splitlines() if s.startswith("{")]
    assert sorted(d["rank"] for d in lines) == [0, 1]
    assert {d["world_size"] for d in lines} == {2}
    assert sorted(d["local_rank"] for d in lines) == [0, 1]


def test_world_size_mismatch_is_refused():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"],
                         capture_output=True, text=True, timeout=120,
                         env=_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"))
    assert out.returncode == 2
    assert "WORLD_SIZE=2" in out.stderr


def test_single_rank_dry_launch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-launch"],
                         capture_output=True, text=True, timeout=120, env=_env())
    assert out.returncode == 0
    assert json.loads(out.stdout.strip()) == {"rank": 0, "world_size": 1, "local_rank": 0}


def test_cpu_info_counts_usable_cores():
    sys.path.insert(0, ROOT)
    import bench

    info = bench.cpu_info()
    assert 1 <= info["usable"] <= info["affinity"]
    assert info["usable"] == len(os.sched_getaffinity(0)) or info["cgroup_quota_cpus"]


def test_plain_run_is_the_default_and_full_is_an_option():
    sys.path.insert(0, ROOT)
    import bench

    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def test_output_sample_is_fixed_and_within_its_budget():
    """--dump-outputs' obs sample: the same rows on every call (a seeded draw over the stacked row
    index, ascending), every row when they fit, float32."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench

    a = torch.arange(40 * 6, dtype=torch.float32).view(40, 6)
    b = torch.arange(40 * 6, 70 * 6, dtype=torch.float32).view(30, 6)
    whole = bench._sample_rows([a, b])
    assert whole.dtype == np.float32 and np.array_equal(whole, torch.cat([a, b]).numpy())
    s1 = bench._sample_rows([a, b], budget=10 * 6 * 4)
    s2 = bench._sample_rows([a, b], budget=10 * 6 * 4)
    assert s1.shape == (10, 6) and np.array_equal(s1, s2)
    rows = (s1[:, 0] / 6).astype(int)
    assert np.all(np.diff(rows) > 0) and np.array_equal(s1, torch.cat([a, b]).numpy()[rows])
    assert rows.min() < 40 <= rows.max()  # rows of both blocks (this seed's draw)
    u8 = torch.arange(200, dtype=torch.uint8).view(-1, 1)
    assert np.array_equal(bench._sample_rows([u8])[:, 0], np.arange(200, dtype=np.float32))
