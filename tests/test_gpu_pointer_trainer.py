"""The device evaluate/train loop with `PointerMaskedAgent(fused_pointer=True)` on MI355X: the
fused pointer heads (nmmo_amd/heads.py `pointer_heads`, SPEC.md §18) between the engine's obs rows
and `nmmo_step`, with the reference's decoder shape: keys from the row's Entity, Inventory and
Market sections, one query per pointer head. The shape is test_gpu_heads_trainer.py's (C4,
MAP_N=2, 2 envs, batch_size 1024, batch_rows 16, hidden 64), and so is the rule for float
comparisons: the fused path's error against a float64 reference stays within 4 x the error of the
unfused float32 torch chain (`cat` of a zero row, `matmul`, the loop of Categoricals) against it."""

import copy

import numpy as np
import pytest
import torch

from tests.conftest import gpu_available
from tests.test_gpu_heads import closed_form, head_slices, within

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

_runs = {}
# Ticks before the stored batch. On the first ticks after a reset nobody is in range, owns an item
# or has listed one: every pointer head then has the no-op alone and the keys and queries get no
# gradient. From tick 17 on about half the rows see an attackable entity and some hold items.
WARMUP = 16


def run(tag):
    """One evaluate() (every store also evaluated by unfused copies) and one train(); cached."""
    if tag in _runs:
        return _runs[tag]
    from nmmo_amd.config import Config
    from nmmo_amd.engine import NmmoEngine
    from nmmo_amd.trainer import DeviceTrainer, PointerMaskedAgent, TrainConfig

    torch.manual_seed(0)
    cfg = Config.preset("C4", MAP_N=2, early_stop_agent_num=8)
    eng = NmmoEngine(cfg, 2, seed=5)
    eng.reset()
    agent = PointerMaskedAgent(cfg.TASK_EMBED_DIM, hidden=64, fused_pointer=True, seed=9).cuda()
    unfused = PointerMaskedAgent(cfg.TASK_EMBED_DIM, hidden=64).cuda()
    unfused.load_state_dict(agent.state_dict())
    unfused64 = copy.deepcopy(unfused).double()
    logits64 = []
    masked64 = unfused64.masked
    unfused64.masked = lambda logits, *rest: (logits64.append(logits.detach().cpu().numpy()), masked64(logits, *rest))[1]
    tc = TrainConfig(batch_size=1024, batch_rows=16, bptt_horizon=8, update_epochs=2, total_timesteps=4096)
    tr = DeviceTrainer(eng, agent, tc)
    total = sum(agent.dims)
    n_rows = eng.n_envs * eng.P
    for _ in range(WARMUP):  # the agent's own rollout, not stored
        with torch.no_grad():
            actions, _, _, _ = agent(eng.obs.view(n_rows, eng.obs_elems))
        eng.step(actions.view(eng.n_envs, eng.P, -1))
    seen = {"legal": [], "actions": [], "fused": [], "unfused": []}

    def on_store(o, r, d, mask, actions, logprob, value, env_id, step):
        assert actions.dtype == torch.int32
        with torch.no_grad():
            _, lp_unfused, _, _ = unfused(o, action=actions.long())
            unfused64(o.double(), action=actions.long())
        seen["legal"].append((o[:, :total] > 0).cpu().numpy())
        seen["actions"].append(actions.cpu().numpy())
        seen["fused"].append(logprob.double().cpu().numpy())
        seen["unfused"].append(lp_unfused.double().cpu().numpy())

    stats = tr.evaluate(on_store=on_store)
    exp = tr.experience
    out = {"tc": tc, "stats": stats, "ptr": exp.ptr, "dims": agent.dims, "task_dim": cfg.TASK_EMBED_DIM,
           "draws": agent.draws, "steps": len(seen["fused"]), "seen": {k: np.concatenate(v) for k, v in seen.items()},
           "logits64": np.concatenate(logits64),
           "exp": {k: getattr(exp, k).cpu() for k in ("obs", "actions", "logprobs", "rewards", "dones", "values")},
           "agent_state": copy.deepcopy(agent.state_dict())}
    before = [p.detach().clone() for p in agent.parameters()]
    out["losses"] = tr.train()
    out["moved"] = any(not torch.equal(p0, p1.detach()) for p0, p1 in zip(before, agent.parameters()))
    eng.close()
    _runs[tag] = out
    return out


def test_fused_evaluate_fills_the_batch():
    o = run("a")
    assert o["ptr"] == o["tc"].batch_size + 1
    assert o["stats"]["agent_steps"] >= o["tc"].batch_size + 1 and o["stats"]["agent_SPS"] > 0
    assert o["draws"] == WARMUP + o["steps"]  # the draw counter advanced once per sampling call


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
    o = run("a")
    s = o["seen"]
    # float64: §15's closed form on the float64 copy's materialised logits
    want, _, _, _ = closed_form(o["logits64"], s["legal"], o["dims"], s["actions"])
    print(f"logits: max |x| {np.abs(o['logits64']).max():.2f}")
    within("evaluate logprob", s["fused"], want, s["unfused"])


def test_minibatch_parameter_gradients_agree():
    from nmmo_amd.trainer import PointerMaskedAgent

    o = run("a")
    obs = o["exp"]["obs"][:128].cuda()
    actions = o["exp"]["actions"][:128].cuda()
    candidates = [int((obs[:, sl.start:sl.stop - 1] > 0).sum()) for sl in head_slices(o["dims"])]
    print(f"legal entries besides the last, per head: {candidates}")
    adv = torch.from_numpy(np.random.default_rng(1).standard_normal(128)).cuda()

    def grads(fused, dtype):
        agent = PointerMaskedAgent(o["task_dim"], hidden=64, fused_pointer=fused).cuda()
        agent.load_state_dict(o["agent_state"])
        agent = agent.to(dtype)
        _, logp, ent, value = agent(obs.to(dtype), action=actions.long())
        loss = -(logp * adv.to(dtype)).mean() - 0.01 * ent.mean() + 0.5 * (value.view(-1) ** 2).mean()
        loss.backward()
        return {k: p.grad.double().cpu().numpy() for k, p in agent.named_parameters()}

    want, g_unfused, g_fused = grads(False, torch.float64), grads(False, torch.float32), grads(True, torch.float32)
    # encoder, value, 3 key encoders, 8 queries, 4 dense heads: weight and bias each
    assert set(want) == set(g_fused) and len(want) == 2 * (1 + 1 + 3 + 8 + 4)
    for name in want:
        within(f"grad {name}", g_fused[name], want[name], g_unfused[name])
    # the rows exercise the pointer heads: entity and inventory keys and their queries get gradients
    # (queries.0 is Attack.Target's, queries.2 Destroy.InventoryItem's; nothing is listed on the market yet)
    for name in ("key_encoders.0.weight", "key_encoders.1.weight", "queries.0.weight", "queries.2.weight"):
        assert np.abs(want[name]).max() > 0, name


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
