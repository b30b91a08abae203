"""The mask pass of the flat rows' mirror variant on MI355X (flat_obs.hip fo_mask_pass):
the tracked ActionTargets chunks, their compare with the row state and the row-state write-back of a
wave's four agents done once per wave, lane = (agent, chunk). Every comparison is bit-exact: against
the CPU oracle (plain runs) and against a handle created under NMMO_FLAT_FUSE=0, whose staging variant
keeps the per-row code. tests/flat_maskpass_states.py builds the states and
tests/test_flat_maskpass_states.py asserts on the CPU that they hold the counts claimed.

Every state is stepped twice with no-op actions over the same buffer. After every step the obs counter
(rows written, bytes stored), the state and the step outputs equal the staging handle's. The row
state itself (NmmoEngine.obs_row_state: the rows whose state is valid, zst, and zext where zst says it
is valid) is compared word for word after every step too, where the library has the read-only hook
that copies it out: the product library exports its public header and nothing else, so the last test
runs this file once more in a process of its own on the hook build (build.HOOKS_PATH: the same
sources with -DNMMO_TEST_HOOKS). Under a wrapper the oracle's rows are the ones OracleWrapper edits
(tests/wrapper_cases.edited_obs, the last price being the step's Sell.Price action).

  1. the lane-group bound: 15 / 16 / 17 / 1 visible rows in one wave, more than 100 beside 1, a
     same-tile attackable player at rows 15 and 16; inventories of 0, 1, 11, 12 items; gold 0, 1, 98,
     99, 100;
  2. 0, 1, 24, 25, 63, 64, 65, 959, 960, 961 listings with own and unaffordable listings at the edges
     of Buy's words;
  3. mixed waves: in the realm, dead for several ticks, dead since this tick, back this tick, Tile
     sections invalidated;
  4. the wrappers' edits (last price 0, 63, 64, 98 and none, no-give, no-dangerous-NPC);
  5. stillness: the second of two no-op steps from a quiet state;
  6. a captured graph of 3 steps replayed equals eager steps."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from nmmo_amd import abi, build
from tests import flat_maskpass_states as ms
from tests import obs_scenarios as sc
from tests import wrapper_cases as wc
from tests.conftest import gpu_available
from tests.test_gpu_obs_saturation import _same

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

N = sc.N_ENVS


def _engine(wrapper=None):
    from nmmo_amd.engine import NmmoEngine
    from nmmo_amd.wrappers import wrapper_config

    eng = NmmoEngine(sc.config(obs_layout=abi.OBS_FLAT), N, seed=3)
    sc.set_tasks(eng, 128)
    if wrapper:
        eng.set_wrapper(wrapper_config(wrapper))
    eng.counter = torch.zeros((N, 2), dtype=torch.int64, device=eng.device)
    eng.set_obs_counter(eng.counter)
    return eng


def _pair(monkeypatch, wrapper=None):
    """(mirror, staged): the second created under NMMO_FLAT_FUSE=0."""
    monkeypatch.delenv("NMMO_FLAT_FUSE", raising=False)
    a = _engine(wrapper)
    monkeypatch.setenv("NMMO_FLAT_FUSE", "0")
    b = _engine(wrapper)
    monkeypatch.delenv("NMMO_FLAT_FUSE")
    return a, b


ZS_EXT = np.uint64(1 << 21)  # kernels.h kZsExt: the row's zext words are valid
ON_HOOK_BUILD = os.environ.get("NMMO_LIB") == build.HOOKS_PATH  # (test_row_state_... below starts that process)


def _row_state(a, b, name, errs):
    (va, sa, xa), (vb, sb, xb) = a.obs_row_state(), b.obs_row_state()
    if not va.all() or not np.array_equal(va, vb):
        errs.append(f"{name}: rows with a valid state {int(va.sum())} (mirror), {int(vb.sum())} (staged) of {va.size}")
        return
    if not np.array_equal(sa, sb):
        bad = np.argwhere(sa != sb)
        errs.append(f"{name}: zst differs at {bad.shape[0]} rows, first (env, agent) {bad[0].tolist()}: "
                    f"{int(sa[tuple(bad[0])]):#x} != staged {int(sb[tuple(bad[0])]):#x}")
        return
    ext = (sa & ZS_EXT) != 0
    if not np.array_equal(xa[ext], xb[ext]):
        bad = np.argwhere((xa != xb) & ext[:, :, None])
        e, p, k = bad[0].tolist()
        errs.append(f"{name}: zext differs at {bad.shape[0]} words, first (env, agent, word) {(e, p, k)}: "
                    f"{int(xa[e, p, k]):#x} != staged {int(xb[e, p, k]):#x}")


def _walk(a, b, orc, steps, wrapper=None):
    """steps: (name, blob or None, actions, invalidate the Tile sections first). The obs counters are
    compared as deltas per step; returns them."""
    errs, deltas = [], []
    for name, blob, acts, inval in steps:
        before = a.counter.clone(), b.counter.clone()
        for h in (a, b, orc):
            if blob is not None:
                h.set_state(blob)
            if h is orc:
                h.step(acts)
            else:
                if inval:
                    h.obs_invalidate_sections(abi.OBS_SEC_TILE)
                h.step(torch.from_numpy(acts).to(h.device))
        torch.cuda.synchronize()
        _same(a.obs, b.obs.reshape(N, a.P, -1), f"{name}: mirror vs staged", errs)
        want = orc.obs if wrapper is None else wc.edited_obs(orc, wrapper, {}, prev_price=acts[:, :, ms.HEAD["Sell.Price"]])[1]
        _same(a.obs, torch.from_numpy(want).to(a.device), f"{name}: mirror vs oracle", errs)
        if ON_HOOK_BUILD:
            _row_state(a, b, name, errs)
        da, db = (a.counter - before[0]).tolist(), (b.counter - before[1]).tolist()
        if da != db:
            errs.append(f"{name}: obs counter {da} != staged {db}")
        if not np.array_equal(a.get_state(), b.get_state()):
            errs.append(f"{name}: state differs from the staged handle's")
        for k in ("rew", "term", "trunc", "mask"):
            if not torch.equal(getattr(a, k), getattr(b, k)):
                errs.append(f"{name}: {k} differs")
        deltas.append(da)
    assert not errs, "\n".join(errs)
    assert a.get_fault() == 0 and b.get_fault() == 0
    return deltas


def _twice(states, acts):
    out = []
    for name, blob in states:
        out += [(name, blob, acts, False), (name + ", again", None, acts, False)]
    return out


def test_lane_group_bound(monkeypatch):
    a, b = _pair(monkeypatch)
    orc = sc.make_oracle(sc.config())
    _walk(a, b, orc, _twice(ms.group_states(), ms.noop_actions()))
    a.close()
    b.close()


def test_listing_counts(monkeypatch):
    a, b = _pair(monkeypatch)
    orc = sc.make_oracle(sc.config())
    # up and then down again: the Buy entries and Market rows of the larger counts are cleared
    st = ms.listing_states()
    _walk(a, b, orc, _twice(st + st[-2::-2], ms.noop_actions()))
    a.close()
    b.close()


def test_mixed_waves(monkeypatch):
    a, b = _pair(monkeypatch)
    orc = sc.make_oracle(sc.config())
    allin, out = ms.mixed_states()
    acts = ms.noop_actions()
    _walk(a, b, orc, [
        ("everyone in", allin, acts, False),
        ("again", None, acts, False),
        ("a group, a wave slice and singles died this tick", out, acts, False),
        ("dead since a tick", None, acts, False),
        ("dead, their Tile sections invalidated", None, acts, True),
        ("dead since several ticks", None, acts, False),
        ("back this tick: the row state says zero rows", allin, acts, False),
        ("in the realm, Tile sections invalidated", None, acts, True),
        ("gone again with the Tile sections invalidated", out, acts, True),
    ])
    a.close()
    b.close()


@pytest.mark.parametrize("wrapper", ["neurips23_start_kit", "takeru", "yaofeng"])
def test_wrapper_edits(wrapper, monkeypatch):
    a, b = _pair(monkeypatch, wrapper)
    priced, quiet = ms.noop_actions(prices=True), ms.noop_actions()
    (_, groups), = ms.group_states()
    (_, few), (_, many) = ms.danger_state(), ms.listing_states()[3]
    orc = sc.make_oracle(sc.config())
    _walk(a, b, orc, [
        ("lane groups, last price 0 / 63 / 64 / 98 per wave", groups, priced, False),
        ("again", None, priced, False),
        ("last price 0", None, quiet, False),
        ("listings 24 | 25 with dangerous NPCs, last prices", few, priced, False),
        ("again", None, priced, False),
        ("listings 65 | 959, last price 0", many, quiet, False),
        ("last prices", None, priced, False),
    ], wrapper)
    a.close()
    b.close()


def test_stillness(monkeypatch):
    a, b = _pair(monkeypatch)
    (_, blob), = ms.group_states()
    acts = ms.noop_actions()
    d = _walk(a, b, sc.make_oracle(sc.config()), [("quiet", blob, acts, False), ("still", None, acts, False), ("still", None, acts, False)])
    # (equal to the staging handle's, checked by the walk) and far fewer bytes than the first step's
    assert all(x[1] < y[1] for x, y in zip(d[2], d[0])), d
    a.close()
    b.close()


def test_graph_of_three_steps_equals_eager():
    a, b = _engine(), _engine()
    blob = ms.listing_states()[3][1]

    def steps(e, k):
        for _ in range(k):
            e.scripted_actions(77)
            e.step()

    for e in (a, b):
        e.set_state(blob)
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
        _same(a.obs, b.obs.reshape(N, a.P, -1), f"replay {r}")
        assert torch.equal(a.counter, b.counter), r
    assert np.array_equal(a.get_state(), b.get_state())
    assert a.get_fault() == 0 and b.get_fault() == 0
    a.close()
    b.close()


@pytest.mark.skipif(ON_HOOK_BUILD, reason="this is that process")
def test_row_state_word_for_word_on_the_hook_build():
    """Every test above once more on the hook build, where _walk also compares zst / zext of the
    mirror and the staged handle after every step."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                       cwd=root, env=dict(os.environ, NMMO_LIB=build.HOOKS_PATH), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " passed" in r.stdout and "1 skipped" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
