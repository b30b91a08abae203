"""The device evaluate/train loop with `MaskedLinearAgent(fused_heads=True)` on MI355X: the
fused action heads (nmmo_amd/heads.py) between the engine's obs rows and `nmmo_step`. The shape
is test_gpu_trainer.py's (C4, MAP_N=2, 2 envs, batch_size 1024, batch_rows 16). Float
comparisons follow test_gpu_heads.py's rule: the fused path's error against a float64 reference
stays within 4 x the error of the unfused float32 torch expressions against it."""

import copy

import numpy as np
import pytest
import torch

from tests.conftest import gpu_available
from tests.test_gpu_heads import closed_form, head_slices, within

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

_runs = {}


def run(tag):
    """One evaluate() (checked store by store) and one train() with the fused agent; cached."""
    if tag in _runs:
        return _runs[tag]
    from nmmo_amd.config import Config
    from nmmo_amd.engine import NmmoEngine
    from nmmo_amd.trainer import DeviceTrainer, MaskedLinearAgent, TrainConfig
    from oracle.storage import ReferenceStorage

    torch.manual_seed(0)
    cfg = Config.preset("C4", MAP_N=2, early_stop_agent_num=8)
    eng = NmmoEngine(cfg, 2, seed=5)
    eng.reset()
    agent = MaskedLinearAgent(cfg.TASK_EMBED_DIM, fused_heads=True, seed=9).cuda()
    unfused = MaskedLinearAgent(cfg.TASK_EMBED_DIM).cuda()
    unfused.load_state_dict(agent.state_dict())
    tc = TrainConfig(batch_size=1024, batch_rows=16, bptt_horizon=8, update_epochs=2, total_timesteps=4096)
    tr = DeviceTrainer(eng, agent, tc)
    ref = ReferenceStorage(tc.batch_size, eng.obs_elems)
    total = sum(agent.dims)
    seen = {"logits": [], "legal": [], "actions": [], "fused": [], "unfused": []}
    last_logits = []
    hook = agent.actor.register_forward_hook(lambda mod, inp, out: last_logits.append(out.detach()))

    def on_store(o, r, d, mask, actions, logprob, value, env_id, step):
        ref.store(o.cpu().numpy(), r.cpu(), d.cpu(), mask.cpu().numpy(), actions.cpu().numpy(),
                  logprob.cpu().numpy(), value.cpu().numpy(), env_id.cpu().numpy(), step)
        with torch.no_grad():  # the same rows and shapes through the loop of Categoricals
            _, lp_unfused, _, _ = unfused(o, action=actions.long())
        seen["logits"].append(last_logits[-1].cpu().numpy())
        seen["legal"].append((o[:, :total] > 0).cpu().numpy())
        seen["actions"].append(actions.cpu().numpy())
        seen["fused"].append(logprob.double().cpu().numpy())
        seen["unfused"].append(lp_unfused.double().cpu().numpy())

    stats = tr.evaluate(on_store=on_store)
    hook.remove()
    exp = tr.experience
    out = {"tc": tc, "stats": stats, "ptr": exp.ptr, "ref": ref, "dims": agent.dims, "task_dim": cfg.TASK_EMBED_DIM, "draws": agent.draws,
           "steps": len(seen["fused"]), "seen": {k: np.concatenate(v) for k, v in seen.items()},
           "exp": {k: getattr(exp, k).cpu() for k in ("obs", "actions", "logprobs", "rewards", "dones", "values")},
           "agent_state": copy.deepcopy(agent.state_dict())}
    before = [p.detach().clone() for p in agent.parameters()]
    out["losses"] = tr.train()
    out["moved"] = any(not torch.equal(p0, p1.detach()) for p0, p1 in zip(before, agent.parameters()))
    eng.close()
    _runs[tag] = out
    return out


def test_fused_evaluate_fills_the_batch_and_matches_reference_storage():
    o = run("a")
    assert o["ptr"] == o["tc"].batch_size + 1 == o["ref"].ptr
    assert o["stats"]["agent_steps"] >= o["tc"].batch_size + 1 and o["stats"]["agent_SPS"] > 0
    assert o["draws"] == o["steps"]  # the draw counter advanced once per sampling call
    assert torch.equal(o["exp"]["obs"], o["ref"].obs)
    assert torch.equal(o["exp"]["actions"], o["ref"].actions)
    for name in ("logprobs", "rewards", "dones", "values"):
        assert torch.equal(o["exp"][name], getattr(o["ref"], name)), name


def test_stored_actions_are_legal_under_the_stored_masks():
    o = run("a")
    n = o["ptr"]
    obs, actions = o["exp"]["obs"][:n].numpy(), o["exp"]["actions"][:n].numpy()
    nonempty = 0
    for k, sl in enumerate(head_slices(o["dims"])):
        legal = obs[:, sl] > 0
        has = legal.any(1)
        a = actions[:, k]
        assert np.all((a >= 0) & (a < sl.stop - sl.start))
        assert np.all(legal[np.arange(n), a][has]), k
        nonempty += int(has.sum())
    assert nonempty > n  # the stored rows are living agents with real choices


def test_unfused_agent_reproduces_the_stored_logprobs():
    s = run("a")["seen"]
    want, _, _, _ = closed_form(s["logits"], s["legal"], run("a")["dims"], s["actions"])
    within("evaluate logprob", s["fused"], want, s["unfused"])


def test_minibatch_parameter_gradients_agree():
    from nmmo_amd.trainer import MaskedLinearAgent

    o = run("a")
    obs = o["exp"]["obs"][:128].cuda()
    actions = o["exp"]["actions"][:128].cuda()
    adv = torch.from_numpy(np.random.default_rng(1).standard_normal(128)).cuda()

    def grads(fused, dtype):
        agent = MaskedLinearAgent(o["task_dim"], fused_heads=fused).cuda()
        agent.load_state_dict(o["agent_state"])
        agent = agent.to(dtype)
        _, logp, ent, value = agent(obs.to(dtype), action=actions)
        loss = -(logp * adv.to(dtype)).mean() - 0.01 * ent.mean() + 0.5 * (value.view(-1) ** 2).mean()
        loss.backward()
        return {k: p.grad.double().cpu().numpy() for k, p in agent.named_parameters()}

    want, g_unfused, g_fused = grads(False, torch.float64), grads(False, torch.float32), grads(True, torch.float32)
    assert set(want) == set(g_fused) and len(want) == 6
    for name in want:
        within(f"grad {name}", g_fused[name], want[name], g_unfused[name])


def test_fused_train_moves_the_parameters_with_finite_losses():
    o = run("a")
    for k in ("policy_loss", "value_loss", "entropy", "approx_kl", "clipfrac"):
        assert np.isfinite(o["losses"][k]), k
    assert o["moved"]


def test_same_seeds_give_identical_experience():
    a, b = run("a"), run("b")
    assert a["ptr"] == b["ptr"]
    for name in ("obs", "actions", "logprobs", "rewards", "dones", "values"):
        assert torch.equal(a["exp"][name], b["exp"][name]), name
