"""The device train loop with `TrainConfig(fused_loss=True)` on MI355X: the fused PPO minibatch
loss (nmmo_amd/ppo.py) between the agent's forward and `loss.backward()`. The shape is
test_gpu_heads_trainer.py's (C4, MAP_N=2, 2 envs, batch_size 1024, batch_rows 16). Float
comparisons follow test_gpu_heads.py's rule: the fused path's error against a float64 reference
stays within 4 x the error of the unfused float32 torch expressions against it."""

import copy
import math
import sys

import numpy as np
import pytest
import torch

from tests.conftest import gpu_available
from tests.test_gpu_heads import within

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

KEYS = {"policy_loss", "value_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac", "explained_variance",
        "train_time", "train_sps"}
_runs = {}


def run(fused_loss, fused_heads=False, target_kl=None):
    """One evaluate() and one train(); cached per variant."""
    key = (fused_loss, fused_heads, target_kl)
    if key in _runs:
        return _runs[key]
    from nmmo_amd.config import Config
    from nmmo_amd.engine import NmmoEngine
    from nmmo_amd.trainer import DeviceTrainer, MaskedLinearAgent, TrainConfig

    torch.manual_seed(0)
    cfg = Config.preset("C4", MAP_N=2, early_stop_agent_num=8)
    eng = NmmoEngine(cfg, 2, seed=5)
    eng.reset()
    try:
        agent = MaskedLinearAgent(cfg.TASK_EMBED_DIM, fused_heads=fused_heads, seed=9).cuda()
        tc = TrainConfig(batch_size=1024, batch_rows=16, bptt_horizon=8, update_epochs=2, total_timesteps=4096,
                         fused_loss=fused_loss, target_kl=target_kl)
        tr = DeviceTrainer(eng, agent, tc)
        tr.evaluate()
        out = {"tc": tc, "task_dim": cfg.TASK_EMBED_DIM, "agent_state": copy.deepcopy(agent.state_dict())}
        before = [p.detach().clone() for p in agent.parameters()]
        steps = []
        opt_step = tr.optimizer.step
        tr.optimizer.step = lambda *a, **k: (steps.append(1), opt_step(*a, **k))[1]
        out["losses"] = tr.train()
        out["steps"] = len(steps)
        out["moved"] = any(not torch.equal(p0, p1.detach()) for p0, p1 in zip(before, agent.parameters()))
        idxs, advantages, b = tr.last_batch
        m = tr.experience.minibatch(b["b_idxs"], 0)
        out["minibatch"] = {
            "obs": m["obs"].reshape(-1, tr.experience.obs_elems).clone(),
            "actions": m["actions"].reshape(-1, m["actions"].shape[-1]).clone(),
            "logprobs": m["logprobs"].reshape(-1).clone(), "values": b["b_values"][0].reshape(-1).clone(),
            "advantages": b["b_advantages"][0].reshape(-1).clone(), "returns": b["b_returns"][0].reshape(-1).clone()}
    finally:
        eng.close()
    _runs[key] = out
    return out


def unfused_loss(cfg, newlogprob, entropy, newvalue, old_logprob, mb_advantages, mb_returns, mb_values):
    """The expressions of DeviceTrainer.train's default path."""
    logratio = newlogprob - old_logprob
    ratio = logratio.exp()
    if cfg.norm_adv:
        mb_advantages = (mb_advantages - mb_advantages.mean()) / (mb_advantages.std() + 1e-8)
    pg_loss1 = -mb_advantages * ratio
    pg_loss2 = -mb_advantages * torch.clamp(ratio, 1 - cfg.clip_coef, 1 + cfg.clip_coef)
    pg_loss = torch.max(pg_loss1, pg_loss2).mean()
    newvalue = newvalue.view(-1)
    v_loss_unclipped = (newvalue - mb_returns) ** 2
    v_clipped = mb_values + torch.clamp(newvalue - mb_values, -cfg.vf_clip_coef, cfg.vf_clip_coef)
    v_loss_clipped = (v_clipped - mb_returns) ** 2
    v_loss = 0.5 * torch.max(v_loss_unclipped, v_loss_clipped).mean()
    return pg_loss - cfg.ent_coef * entropy.mean() + v_loss * cfg.vf_coef


def test_minibatch_parameter_gradients_agree():
    """One real minibatch of an evaluate() batch, the agent's parameter gradients three ways."""
    from nmmo_amd.ppo import ppo_loss
    from nmmo_amd.trainer import MaskedLinearAgent

    o = run(True)
    cfg, mb = o["tc"], o["minibatch"]
    assert cfg.norm_adv and cfg.clip_vloss and mb["obs"].shape[0] == 128
    # The old log-probs are the evaluated agent's own, detached, moved by `shift` so that the
    # ratios are exp(-shift) on both sides of the clip in every dtype. (The stored float32 ones
    # would not do for the float64 run: a row's empty heads add 0 to a float32 log-prob and
    # -log n to a float64 one, SPEC §15, which would put every float64 ratio far below the clip.)
    shift = torch.from_numpy(np.random.default_rng(1).standard_normal(128) * 0.1).cuda()

    def grads(fused, dtype):
        agent = MaskedLinearAgent(o["task_dim"]).cuda()
        agent.load_state_dict(o["agent_state"])
        agent = agent.to(dtype)
        _, logp, ent, value = agent(mb["obs"].to(dtype), action=mb["actions"])
        consts = [logp.detach() + shift.to(dtype)] + [mb[k].to(dtype) for k in ("advantages", "returns", "values")]
        if fused:
            loss, _ = ppo_loss(logp, ent, value.view(-1), *consts, clip_coef=cfg.clip_coef,
                               vf_clip_coef=cfg.vf_clip_coef, ent_coef=cfg.ent_coef, vf_coef=cfg.vf_coef,
                               norm_adv=cfg.norm_adv, clip_vloss=cfg.clip_vloss)
        else:
            loss = unfused_loss(cfg, logp, ent, value, *consts)
        loss.backward()
        return {k: p.grad.double().cpu().numpy() for k, p in agent.named_parameters()}

    want, g_unfused, g_fused = grads(False, torch.float64), grads(False, torch.float32), grads(True, torch.float32)
    assert set(want) == set(g_fused) and len(want) == 6
    for name in want:
        assert np.any(want[name] != 0), name
        within(f"grad {name}", g_fused[name], want[name], g_unfused[name])


@pytest.mark.parametrize("fused_heads", [False, True])
def test_fused_train_returns_the_default_keys_and_moves_the_parameters(fused_heads):
    base, o = run(False), run(True, fused_heads)
    assert set(o["losses"]) == set(base["losses"]) == KEYS
    for k, v in o["losses"].items():
        assert math.isfinite(v), k
    assert o["moved"]
    assert o["steps"] == base["steps"] == 2 * 8  # update_epochs x minibatches
    assert 0 <= o["losses"]["clipfrac"] <= 1 and o["losses"]["entropy"] > 0 and o["losses"]["value_loss"] > 0


def test_target_kl_zero_stops_after_the_first_epoch():
    o = run(True, target_kl=0.0)
    assert o["steps"] == 8 and o["moved"]
    assert o["losses"]["approx_kl"] > 0


def test_default_path_does_not_load_the_library(monkeypatch):
    """With nmmo_amd.ppo made unimportable, train() with fused_loss=False runs as ever, and with
    fused_loss=True it fails: the default path never reaches for libnmmo_ppo.so."""
    import nmmo_amd
    from nmmo_amd import ppo

    def refuse():
        raise AssertionError("libnmmo_ppo.so was asked for")

    monkeypatch.setattr(ppo, "lib", refuse)
    monkeypatch.delattr(nmmo_amd, "ppo", raising=False)
    monkeypatch.setitem(sys.modules, "nmmo_amd.ppo", None)
    o = run(False, target_kl=1e9)  # a variant of its own: not served from the cache
    assert o["steps"] == 16 and o["moved"]
    with pytest.raises(ImportError):
        run(True, target_kl=1e9)
