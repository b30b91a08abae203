"""The device train loop with a recurrent agent on MI355X: `RecurrentMaskedAgent(fused_lstm=True,
fused_heads=True)` through `DeviceTrainer.evaluate()` (one LSTM state per agent slot, updated in
place by nml_cell) and `train()` (bptt windows through nml_seq_forward / nml_seq_backward, the
state handed from one minibatch to the next). 2 envs of C4 with MAP_N=4, batch_size 1024,
bptt_horizon 8.

Float comparisons follow test_gpu_heads.py's rule: the error against a float64 CPU copy of the
agent (torch.nn.LSTM, the same state_dict) stays within 4 x the error of its float32 CPU copy.
The float64 log-probs are SPEC §15's closed form (`closed_form`): an empty head adds 0, which a
float64 Categorical over `-1e9` logits does not give."""

import copy
import math

import numpy as np
import pytest
import torch

from tests.conftest import gpu_available
from tests.test_gpu_heads import closed_form, within
from tests.test_gpu_ppo_trainer import KEYS

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

HIDDEN = 64
_runs = {}


def run(fused_loss=False, batch_rows=128, record=False):
    """One evaluate() and one train() of the fused recurrent agent; cached per variant."""
    key = (fused_loss, batch_rows, record)
    if key in _runs:
        return _runs[key]
    from nmmo_amd.config import Config
    from nmmo_amd.engine import NmmoEngine
    from nmmo_amd.trainer import DeviceTrainer, RecurrentMaskedAgent, TrainConfig

    torch.manual_seed(0)
    cfg = Config.preset("C4", MAP_N=4, early_stop_agent_num=8)
    eng = NmmoEngine(cfg, 2, seed=5)
    eng.reset()
    try:
        agent = RecurrentMaskedAgent(cfg.TASK_EMBED_DIM, hidden=HIDDEN, fused_lstm=True, fused_heads=True, seed=9).cuda()
        tc = TrainConfig(batch_size=1024, batch_rows=batch_rows, bptt_horizon=8, update_epochs=1, total_timesteps=4096,
                         fused_loss=fused_loss)
        tr = DeviceTrainer(eng, agent, tc)
        state0 = tr.next_lstm_state
        out = {"tc": tc, "task_dim": cfg.TASK_EMBED_DIM, "n_rows": tr.n_rows, "dims": agent.dims,
               "state0": tuple(t.clone() for t in state0), "state_ptrs": tuple(t.data_ptr() for t in state0)}
        seen = []
        tr.evaluate(on_store=lambda o, *rest: seen.append(o.cpu()))
        out["obs_steps"] = seen
        out["state"] = tuple(t.cpu() for t in tr.next_lstm_state)
        out["state_is_same_tensors"] = all(a is b for a, b in zip(tr.next_lstm_state, state0))
        out["agent_state"] = copy.deepcopy({k: v.cpu() for k, v in agent.state_dict().items()})
        calls = []
        if record:
            forward = agent.forward

            def recording(obs, state=None, action=None):
                res = forward(obs, state=state, action=action)
                calls.append({"obs_shape": tuple(obs.shape), "state": state, "returned": res[4]})
                return res

            agent.forward = recording
        out["losses"] = tr.train()
        out["calls"] = calls
        out["moved"] = {k: not torch.equal(v.cpu(), out["agent_state"][k]) for k, v in agent.state_dict().items()}
        idxs, advantages, b = tr.last_batch
        m = tr.experience.minibatch(b["b_idxs"], 0)
        out["minibatch"] = {
            "obs": m["obs"].reshape(tc.batch_rows, tc.bptt_horizon, tr.experience.obs_elems).cpu(),
            "actions": m["actions"].reshape(-1, m["actions"].shape[-1]).cpu(),
            "logprobs": m["logprobs"].reshape(-1).cpu(), "values": b["b_values"][0].reshape(-1).cpu(),
            "advantages": b["b_advantages"][0].reshape(-1).cpu(), "returns": b["b_returns"][0].reshape(-1).cpu()}
        out["num_minibatches"] = b["num_minibatches"]
    finally:
        eng.close()
    _runs[key] = out
    return out


def cpu_copy(o, dtype):
    """The agent with torch.nn.LSTM and the loop of Categoricals, on the CPU in `dtype`."""
    from nmmo_amd.trainer import RecurrentMaskedAgent

    agent = RecurrentMaskedAgent(o["task_dim"], hidden=HIDDEN)
    agent.load_state_dict(o["agent_state"])
    return agent.to(dtype)


def test_evaluate_and_train_run_and_return_the_default_keys():
    o = run()
    assert set(o["losses"]) == KEYS
    for k, v in o["losses"].items():
        assert math.isfinite(v), k
    assert o["num_minibatches"] == 1 and len(o["obs_steps"]) >= 4
    lstm_keys = [k for k in o["moved"] if k.startswith("lstm.")]
    assert sorted(lstm_keys) == ["lstm.bias_hh_l0", "lstm.bias_ih_l0", "lstm.weight_hh_l0", "lstm.weight_ih_l0"]
    assert all(o["moved"][k] for k in lstm_keys), o["moved"]


def test_evaluate_carries_one_state_per_agent_slot():
    """Zero at the start, [num_layers, n_rows, hidden], updated in place, and equal to the float64
    CPU agent stepped from zero state over the observations evaluate() saw."""
    o = run()
    for t in o["state0"]:
        assert tuple(t.shape) == (1, o["n_rows"], HIDDEN) and t.dtype == torch.float32 and not t.any()
    assert o["state_is_same_tensors"]
    results = {}
    for dtype in (torch.float64, torch.float32):
        agent, state = cpu_copy(o, dtype), None
        with torch.no_grad():
            for obs in o["obs_steps"]:
                _, _, state = agent.hidden(obs.to(dtype), state)
        results[dtype] = [t.double().numpy() for t in state]
    for name, got, want, ref in zip("hc", o["state"], results[torch.float64], results[torch.float32]):
        assert np.abs(want).max() > 1e-3
        within(f"next_lstm_state {name}", got.double().numpy(), want, ref)


def losses_of(o, dtype):
    """policy and value loss of the minibatch from a CPU copy of the agent evaluated on the
    [batch_rows, bptt_horizon, obs] window with state=None: DeviceTrainer.train's default
    expressions (test_gpu_ppo_trainer.py's `unfused_loss`)."""
    cfg, mb = o["tc"], o["minibatch"]
    agent = cpu_copy(o, dtype)
    with torch.no_grad():
        if dtype == torch.float64:
            h, flat, _ = agent.hidden(mb["obs"].to(dtype), None)
            legal = (flat[:, :sum(agent.dims)] > 0).numpy()
            logp, _, _, _ = closed_form(agent.actor(h).numpy(), legal, agent.dims, mb["actions"].numpy())
            newlogprob, newvalue = torch.from_numpy(logp), agent.value(h).view(-1)
        else:
            _, newlogprob, _, newvalue, _ = agent(mb["obs"], state=None, action=mb["actions"].long())
            newvalue = newvalue.view(-1)
        old_logprob, mb_advantages, mb_returns, mb_values = (mb[k].to(dtype) for k in ("logprobs", "advantages",
                                                                                       "returns", "values"))
        ratio = (newlogprob - old_logprob).exp()
        mb_advantages = (mb_advantages - mb_advantages.mean()) / (mb_advantages.std() + 1e-8)
        pg_loss1 = -mb_advantages * ratio
        pg_loss2 = -mb_advantages * torch.clamp(ratio, 1 - cfg.clip_coef, 1 + cfg.clip_coef)
        pg_loss = torch.max(pg_loss1, pg_loss2).mean()
        v_loss_unclipped = (newvalue - mb_returns) ** 2
        v_clipped = mb_values + torch.clamp(newvalue - mb_values, -cfg.vf_clip_coef, cfg.vf_clip_coef)
        v_loss_clipped = (v_clipped - mb_returns) ** 2
        v_loss = 0.5 * torch.max(v_loss_unclipped, v_loss_clipped).mean()
    return {"policy_loss": float(pg_loss), "value_loss": float(v_loss)}


@pytest.mark.parametrize("fused_loss", [False, True])
def test_train_losses_match_the_float64_agent(fused_loss):
    o = run(fused_loss)
    assert o["tc"].norm_adv and o["tc"].clip_vloss and o["minibatch"]["obs"].shape[:2] == (128, 8)
    want, ref = losses_of(o, torch.float64), losses_of(o, torch.float32)
    for k in ("policy_loss", "value_loss"):
        within(f"{k} fused_loss={fused_loss}", np.array([o["losses"][k]]), np.array([want[k]]), np.array([ref[k]]))


def test_second_minibatch_receives_the_detached_state():
    o = run(batch_rows=64, record=True)
    calls = o["calls"]
    assert o["num_minibatches"] == 2 and len(calls) == 2
    assert all(c["obs_shape"][:2] == (64, 8) for c in calls)
    assert calls[0]["state"] is None
    state = calls[1]["state"]
    assert state is not None and len(state) == 2
    for got, sent in zip(state, calls[0]["returned"]):
        assert tuple(got.shape) == (1, 64, HIDDEN)
        assert not got.requires_grad and got.grad_fn is None
        assert sent.requires_grad  # what the agent returned was attached; train() detached it
        assert torch.equal(got, sent.detach())


def test_non_recurrent_trainer_has_no_lstm_state():
    from nmmo_amd.config import Config
    from nmmo_amd.engine import NmmoEngine
    from nmmo_amd.trainer import DeviceTrainer, MaskedLinearAgent, TrainConfig

    cfg = Config.preset("C4", MAP_N=4, early_stop_agent_num=8)
    eng = NmmoEngine(cfg, 2, seed=5)
    try:
        tr = DeviceTrainer(eng, MaskedLinearAgent(cfg.TASK_EMBED_DIM).cuda(), TrainConfig(batch_size=1024))
        assert tr.next_lstm_state is None
    finally:
        eng.close()
