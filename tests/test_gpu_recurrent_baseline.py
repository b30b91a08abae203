"""`baseline.RecurrentBaselineAgent`, the start-kit `Recurrent(Baseline)`, on MI355X with every flag on
(`fused_decoder`, `fused_lstm`, the fused encoders), two LSTM layers, and `rollout.run_policy`.

The shape is test_gpu_baseline_trainer.py's: C4, MAP_N=2, 2 envs (256 rows), hidden 64, a random task
embedding, `query_scale = 1 / sqrt(hidden)` and its state edit (the players pairwise on one tile with 99
gold, past their immunity, one listed and one unlisted item each), applied straight after the reset so
that two engines made from one seed are in the same state; the legal entries per pointer head on the
rows the tests start from are asserted non-zero for all eight.

  - Twins: an agent with the same `state_dict` and `fused_decoder=False` (`item_logits`, `player_logits`,
    `cat`, `masked_heads`; SPEC.md §23 makes the two the same bits) re-evaluates the sampled actions to
    the same logprob bits and selects the same greedy actions, over 4 steps that carry the LSTM state.
  - Float: the project's rule, tests/test_gpu_heads.py `within`. Against a float64 copy on the host
    (`nn.LSTM`, test_gpu_heads.py's closed form on its float64 logits), the fused agent's logprob, value
    and LSTM state over the 4 steps err at most 4 x what an unfused float32 copy on the GPU (`nn.LSTM`)
    errs; and so does a [B, 4, E] window with the actions given (grad mode: the sequence kernels)
    against the same float64 values. Logprob is compared on the rows none of whose heads is empty:
    torch gives an empty head -log n where §15 gives 0, which is no rounding error.
  - `DeviceTrainer` (batch_size 1024, batch_rows 16, bptt_horizon 8): `next_lstm_state` is [2, 256, 64]
    and updated in place, `train()` has finite losses and moves every `recurrent.*` parameter and
    `policy.proj_fc.*`, and the forward leaves the engine's obs rows unchanged.
  - `run_policy`, 16 steps: greedy runs on two engines from one seed give the same actions at every
    step and the same `reward_sum`, also from an agent built with another philox seed, and draw
    nothing; sampled runs under the two seeds differ.
"""

import math

import numpy as np
import pytest
import torch

from tests.conftest import gpu_available
from tests.test_gpu_baseline_trainer import FUSED, POINTER
from tests.test_gpu_heads import closed_form, within

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

HIDDEN, LAYERS, STEPS = 64, 2, 4
SCALE = 1.0 / math.sqrt(HIDDEN)
SEEDS = (9, 10)  # philox seeds of the two agents of the run_policy test: their sampled runs differ (checked there)


def make_engine():
    """The engine of test_gpu_baseline_trainer.py after its state edit, without warm-up ticks."""
    from nmmo_amd import abi
    from nmmo_amd.config import Config
    from nmmo_amd.engine import NmmoEngine
    from oracle.oracle import join_state, split_state

    cfg = Config.preset("C4", MAP_N=2, early_stop_agent_num=8)
    task = np.random.default_rng(3).standard_normal(cfg.TASK_EMBED_DIM).astype(np.float16)
    eng = NmmoEngine(cfg, 2, seed=5, task_embedding=task)
    eng.reset()
    state = split_state(eng.get_state(), eng.n_envs, eng.S, eng.P)
    ent, F = state["ent"], abi.F
    ent[:, F["gold"], :eng.P] = 99
    ent[:, F["time_alive"], :eng.P] = np.maximum(ent[:, F["time_alive"], :eng.P], 30)
    for p in range(1, eng.P, 2):
        ent[:, F["row"], p] = ent[:, F["row"], p - 1]
        ent[:, F["col"], p] = ent[:, F["col"], p - 1]
    slots = abi.INV_SLOTS * eng.P
    state["items"][:] = 0
    for e in range(eng.n_envs):
        for p in range(eng.P):
            state["items"][e, p, 0] = [5 | (1 << 5) | (7 << 10), 1 | ((2 * p + 1) << 16)]
            state["items"][e, p, 1] = [16 | (1 << 5), 1 | ((2 * p + 2) << 16)]
        used = 2 * eng.P
        state["iring"][e, :] = 0
        state["iring"][e, :slots - used] = np.arange(used + 1, slots + 1)
        state["env"][e, abi.E["item_free_head"]] = 0
        state["env"][e, abi.E["item_free_count"]] = slots - used
    ent[:, F["item_level"], :eng.P] = 0
    eng.set_state(join_state(state))
    eng.observe()
    return eng, cfg


def make_agent(cfg, seed=9, **flags):
    from nmmo_amd.baseline import RecurrentBaselineAgent

    return RecurrentBaselineAgent(cfg.TASK_EMBED_DIM, HIDDEN, num_layers=LAYERS, seed=seed, query_scale=SCALE, **flags)


ALL_ON = dict(fused_lstm=True, fused_decoder=True, **FUSED)
_steps = {}


def steps():
    """4 sampled steps of the all-flags agent with its twin, the unfused float32 copy and the float64 copy
    alongside, then the same 4 rows as one window; cached."""
    if _steps:
        return _steps
    from nmmo_amd import layout
    from nmmo_amd.baseline import DECODER_LAYERS

    torch.manual_seed(0)
    eng, cfg = make_engine()
    agent = make_agent(cfg, **ALL_ON).cuda()
    with torch.no_grad():  # biases 0 would hide a dropped bias
        for name, p in agent.recurrent.named_parameters():
            if "bias" in name:
                p.uniform_(-0.1, 0.1)
    twin = make_agent(cfg, fused_lstm=True, fused_decoder=False, **FUSED).cuda()
    unfused = make_agent(cfg).cuda()
    exact = make_agent(cfg)
    for other in (twin, unfused, exact):
        other.load_state_dict(agent.state_dict(), strict=True)
    exact = exact.double()
    pol = exact.policy
    n = eng.n_envs * eng.P
    total = sum(pol.dims)
    seen = {k: [] for k in ("lp", "lp_unfused", "lp_want", "v", "v_unfused", "v_want", "h", "h_unfused", "h_want",
                            "c", "c_unfused", "c_want", "full")}
    twin_bits, greedy_same, obs_rows, acts = [], [], [], []
    counts = {name: 0 for name in POINTER}
    st = st_twin = st_unfused = st_exact = None
    with torch.no_grad():
        for _ in range(STEPS):
            o = eng.obs.view(n, eng.obs_elems)
            obs_rows.append(o.clone())
            for name in POINTER:
                k = layout.HEAD[name]
                counts[name] += int((o[:, pol.mask_off[k]:pol.mask_off[k + 1] - 1] > 0).sum())
            # greedy from copies of the states the sampled step starts from (a given state is updated in place)
            copies = [None if s is None else (s[0].clone(), s[1].clone()) for s in (st, st_twin)]
            g_a, g_t = agent(o, copies[0], greedy=True)[0], twin(o, copies[1], greedy=True)[0]
            greedy_same.append(g_a.dtype == torch.int32 and torch.equal(g_a, g_t))
            a, lp, _, v, st = agent(o, st)
            _, lp_twin, _, _, st_twin = twin(o, st_twin, action=a)
            twin_bits.append(torch.equal(lp_twin.view(torch.int32), lp.view(torch.int32)))
            _, lp_u, _, v_u, st_unfused = unfused(o, st_unfused, action=a.long())
            o64 = o.double().cpu()
            h, emb = pol._encode(o64)
            y, st_exact = exact.recurrent(h.unsqueeze(0), st_exact)
            out = [pol.action_decoder.layers[name](y[0]) for name, _ in DECODER_LAYERS]
            logits = pol.logits(out, {k: out[k] * SCALE for k in pol.pointer}, o64, emb)
            legal = (o[:, :total] > 0).cpu().numpy()
            off = np.cumsum([0] + pol.dims)
            seen["full"].append(np.array([all(legal[r, off[k]:off[k + 1]].any() for k in range(12)) for r in range(n)]))
            seen["lp_want"].append(closed_form(logits.numpy(), legal, pol.dims, a.cpu().numpy())[0])
            seen["v_want"].append(pol.value_head(y[0]).flatten().numpy())
            for key, t in (("lp", lp), ("lp_unfused", lp_u), ("v", v.flatten()), ("v_unfused", v_u.flatten()),
                           ("h", st[0]), ("h_unfused", st_unfused[0]), ("h_want", st_exact[0]),
                           ("c", st[1]), ("c_unfused", st_unfused[1]), ("c_want", st_exact[1])):
                seen[key].append(t.double().cpu().numpy().copy())
            acts.append(a.clone())
            eng.step(a.view(eng.n_envs, eng.P, -1))
    eng.check_fault("test_gpu_recurrent_baseline.steps")
    # the same rows as one [B, 4, E] window with the actions given, from a zero state, in grad mode
    window = torch.stack(obs_rows, 1)
    _, w_lp, _, w_v, w_state = agent(window, action=torch.stack(acts, 1))
    by_step = lambda t: t.detach().double().cpu().numpy().reshape(n, STEPS).T  # noqa: E731  (B, T) order -> [T, B]
    _steps.update(seen={k: np.stack(v) for k, v in seen.items()}, twin_bits=twin_bits, greedy_same=greedy_same,
                  counts=counts, draws=agent.draws, w_lp=by_step(w_lp), w_v=by_step(w_v),
                  w_h=w_state[0].detach().double().cpu().numpy(), w_c=w_state[1].detach().double().cpu().numpy())
    eng.close()
    return _steps


def test_the_rows_have_legal_entries_in_all_eight_pointer_heads():
    o = steps()
    print("legal entries besides the no-op: " + ", ".join(f"{v} {k}" for k, v in o["counts"].items()))
    assert len(o["counts"]) == 8 and all(v > 0 for v in o["counts"].values()), o["counts"]
    assert o["seen"]["full"].mean() >= 0.5  # the rows the logprob comparison keeps


def test_the_composed_twin_gives_the_same_logprob_bits_and_the_same_greedy_actions():
    o = steps()
    assert len(o["twin_bits"]) == STEPS and all(o["twin_bits"]), o["twin_bits"]
    assert all(o["greedy_same"]), o["greedy_same"]
    assert o["draws"] == STEPS  # the greedy calls in between drew nothing


def test_steps_stay_within_the_unfused_agents_error():
    s = steps()["seen"]
    assert np.abs(s["v_want"]).max() > 0 and np.abs(s["h_want"]).max() > 0
    within("step logprob", s["lp"], s["lp_want"], s["lp_unfused"], rows=s["full"])
    within("step value", s["v"], s["v_want"], s["v_unfused"])
    within("step h", s["h"], s["h_want"], s["h_unfused"])
    within("step c", s["c"], s["c_want"], s["c_unfused"])


def test_a_window_stays_within_the_unfused_agents_error_of_the_single_steps():
    o = steps()
    s = o["seen"]
    within("window logprob", o["w_lp"], s["lp_want"], s["lp_unfused"], rows=s["full"])
    within("window value", o["w_v"], s["v_want"], s["v_unfused"])
    within("window h", o["w_h"], s["h_want"][-1], s["h_unfused"][-1])
    within("window c", o["w_c"], s["c_want"][-1], s["c_unfused"][-1])


def test_device_trainer_carries_the_state_in_place_and_trains_the_lstm():
    from nmmo_amd.trainer import DeviceTrainer, TrainConfig

    torch.manual_seed(1)
    eng, cfg = make_engine()
    agent = make_agent(cfg, **ALL_ON).cuda()
    tc = TrainConfig(batch_size=1024, batch_rows=16, bptt_horizon=8, update_epochs=1, total_timesteps=4096)
    tr = DeviceTrainer(eng, agent, tc)
    n = eng.n_envs * eng.P
    h, c = tr.next_lstm_state
    assert tuple(h.shape) == tuple(c.shape) == (LAYERS, n, HIDDEN) == (2, 256, 64)
    where = (h.data_ptr(), c.data_ptr())
    before_forward, obs_kept = [], []
    hook = agent.register_forward_pre_hook(lambda mod, args: before_forward.append(args[0].clone()))
    tr.evaluate(on_store=lambda o, *rest: obs_kept.append(torch.equal(o, before_forward[-1])))
    hook.remove()
    assert tr.experience.ptr == tc.batch_size + 1
    assert (tr.next_lstm_state[0].data_ptr(), tr.next_lstm_state[1].data_ptr()) == where
    assert float(tr.next_lstm_state[0].abs().max()) > 0 and float(tr.next_lstm_state[1].abs().max()) > 0
    assert len(obs_kept) >= tc.batch_size // n and all(obs_kept)
    before = {k: p.detach().clone() for k, p in agent.named_parameters()}
    losses = tr.train()
    eng.close()
    for k in ("policy_loss", "value_loss", "entropy", "approx_kl", "clipfrac"):
        assert np.isfinite(losses[k]), k
    moved = {k: not torch.equal(before[k], p.detach()) for k, p in agent.named_parameters()}
    want = [k for k in moved if k.startswith("recurrent.")] + ["policy.proj_fc.weight", "policy.proj_fc.bias"]
    assert len(want) == 4 * LAYERS + 2 and all(moved[k] for k in want), [k for k in want if not moved[k]]


def test_run_policy_is_deterministic_when_greedy_and_not_when_sampling():
    from nmmo_amd.rollout import run_policy

    torch.manual_seed(2)
    agents = None
    runs = {}
    for key, seed_i, greedy in (("g0", 0, True), ("g1", 0, True), ("g_other_seed", 1, True), ("s0", 0, False),
                                ("s_other_seed", 1, False)):
        eng, cfg = make_engine()
        if agents is None:
            agents = [make_agent(cfg, seed=s, **ALL_ON).cuda() for s in SEEDS]
            agents[1].load_state_dict(agents[0].state_dict(), strict=True)
        agent = agents[seed_i]
        agent.draws = 0
        acts = []
        out = run_policy(eng, agent, 16, greedy=greedy, on_step=lambda o, a, lp, v: acts.append(a.clone()))
        eng.close()
        n = eng.n_envs * eng.P
        assert out["steps"] == 16 and len(acts) == 16 and 0 < out["agent_steps"] <= 16 * n
        assert out["reward_sum"].dtype == torch.float32 and tuple(out["reward_sum"].shape) == (n,)
        assert tuple(out["state"][0].shape) == (LAYERS, n, HIDDEN)
        assert agent.draws == (0 if greedy else 16)
        runs[key] = (torch.stack(acts), out["reward_sum"], out["agent_steps"])
    for other in ("g1", "g_other_seed"):
        assert torch.equal(runs["g0"][0], runs[other][0]), other
        assert torch.equal(runs["g0"][1], runs[other][1]) and runs["g0"][2] == runs[other][2], other
    assert any(not torch.equal(a, b) for a, b in zip(runs["s0"][0], runs["s_other_seed"][0]))
    assert not torch.equal(runs["s0"][0], runs["g0"][0])
    # an agent without an LSTM is called as the trainer calls it, and there is no state to return
    eng, cfg = make_engine()
    out = run_policy(eng, agents[0].policy, 2)
    eng.close()
    assert out["state"] is None and out["steps"] == 2 and out["agent_steps"] > 0 and agents[0].policy.draws == 16
