"""The device evaluate/train loop with `PlayerMaskedAgent(fused_player=True, fused_heads=True)` on
MI355X: the player-encoder kernels (nmmo_amd/player.py, SPEC.md §21) reading the Entity section and
the AgentId of the engine's obs rows in place, their logits in front of the fused action heads. The
shape is test_gpu_item_trainer.py's (C4, MAP_N=2, 2 envs, batch_size 1024, batch_rows 16). Every
store is re-evaluated by an unfused float32 copy of the agent on the GPU (embeddings, zero row,
matmul, gather: the reference's way) and by a float64 copy on the host (its logits through
test_gpu_heads.py's float64 closed form of §15), and the fused agent's error against the float64
values stays within 4 x the unfused copy's (`within`).

After the reset no two players share a tile, nobody has gold and spawn immunity keeps players from
attacking each other, so Give.Target and GiveGold.Target have the no-op as their only legal entry. A
head whose only legal entry is the no-op gives its query no gradient, fused or not. So the test first
steps the agent's own rollout for WARMUP ticks, unstored, then puts the players pairwise on one tile
with 99 gold each and past their immunity (get_state / set_state), so that the stored rows hold legal
entities in all three `*.Target` heads and every one of the three queries takes part. The same
edit gives every player one listed and one unlisted item, so that the dense item heads (Buy.MarketItem
among them) have legal entries besides the no-op too and every parameter of the agent gets a
gradient. The counts the stores saw (`attacks`, `gives`, `gold_gives`, `buys`: legal entries besides
the no-op) are asserted to be non-zero: if one of the first three were zero, that head's path would
rest on test_gpu_player.py alone."""

import numpy as np
import pytest
import torch

from tests.conftest import gpu_available
from tests.test_gpu_heads import closed_form, within

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

_run = {}
WARMUP = 8  # ticks before the stored batch: the players have moved and met NPCs
PLAYER_LAYERS = ("player_encoder.", "players.", "my_agent.", "queries.")
TARGETS = {"attacks": "Attack.Target", "gives": "Give.Target", "gold_gives": "GiveGold.Target",
           "buys": "Buy.MarketItem"}


def run():
    """One evaluate() (checked store by store) and one train() with the fused agent; cached."""
    if _run:
        return _run
    from nmmo_amd import abi, layout
    from nmmo_amd.config import Config
    from nmmo_amd.engine import NmmoEngine
    from nmmo_amd.trainer import DeviceTrainer, PlayerMaskedAgent, TrainConfig
    from oracle.oracle import join_state, split_state

    torch.manual_seed(0)
    cfg = Config.preset("C4", MAP_N=2, early_stop_agent_num=8)
    eng = NmmoEngine(cfg, 2, seed=5)
    eng.reset()
    agent = PlayerMaskedAgent(cfg.TASK_EMBED_DIM, fused_heads=True, seed=9, fused_player=True).cuda()
    unfused = PlayerMaskedAgent(cfg.TASK_EMBED_DIM).cuda()
    unfused.load_state_dict(agent.state_dict())
    exact = PlayerMaskedAgent(cfg.TASK_EMBED_DIM)
    exact.load_state_dict(agent.state_dict())
    exact = exact.double()
    tc = TrainConfig(batch_size=1024, batch_rows=16, bptt_horizon=8, update_epochs=2, total_timesteps=4096)
    tr = DeviceTrainer(eng, agent, tc)
    total = sum(agent.dims)
    seen = {k: [] for k in ("logp_fused", "logp_unfused", "logp_want", "value_fused", "value_unfused", "value_want")}
    n_rows = eng.n_envs * eng.P
    for _ in range(WARMUP):  # the agent's own rollout, not stored
        with torch.no_grad():
            actions, _, _, _ = agent(eng.obs.view(n_rows, eng.obs_elems))
        eng.step(actions.view(eng.n_envs, eng.P, -1))
    state = split_state(eng.get_state(), eng.n_envs, eng.S, eng.P)
    ent, F = state["ent"], abi.F
    ent[:, F["gold"], :eng.P] = 99  # everyone can give gold
    ent[:, F["time_alive"], :eng.P] = np.maximum(ent[:, F["time_alive"], :eng.P], 30)  # past spawn immunity
    for p in range(1, eng.P, 2):  # pairs on one tile: Give / GiveGold targets, and Attack targets in range
        ent[:, F["row"], p] = ent[:, F["row"], p - 1]
        ent[:, F["col"], p] = ent[:, F["col"], p - 1]
    slots = abi.INV_SLOTS * eng.P  # every player: a listed spear in slot 0, an unlisted ration in slot 1
    state["items"][:] = 0
    for e in range(eng.n_envs):
        for p in range(eng.P):
            # word 0: type, level << 5, price << 10; word 1: quantity, datastore row << 16
            state["items"][e, p, 0] = [5 | (1 << 5) | (7 << 10), 1 | ((2 * p + 1) << 16)]
            state["items"][e, p, 1] = [16 | (1 << 5), 1 | ((2 * p + 2) << 16)]
        used = 2 * eng.P
        state["iring"][e, :] = 0
        state["iring"][e, :slots - used] = np.arange(used + 1, slots + 1)
        state["env"][e, abi.E["item_free_head"]] = 0
        state["env"][e, abi.E["item_free_count"]] = slots - used
    ent[:, F["item_level"], :eng.P] = 0  # nothing is equipped
    eng.set_state(join_state(state))
    eng.observe()
    before_forward, obs_kept = [], []
    counts = {k: 0 for k in TARGETS}
    hook = agent.register_forward_pre_hook(lambda mod, args: before_forward.append(args[0].clone()))

    def on_store(o, r, d, mask, actions, logprob, value, env_id, step):
        obs_kept.append(torch.equal(o, before_forward[-1]))  # the forward wrote nothing into the obs rows
        with torch.no_grad():
            _, lp_unfused, _, v_unfused = unfused(o, action=actions.long())
            o64 = o.double().cpu()
            h, emb = exact.hidden(o64)
            lp_want = closed_form(exact.logits(h, o64, emb).numpy(), (o[:, :total] > 0).cpu().numpy(),
                                  agent.dims, actions.cpu().numpy())[0]
            v_want = exact.value(h).flatten().numpy()
        for k, name in TARGETS.items():
            off = agent.mask_off[layout.HEAD[name]]
            counts[k] += int((o[:, off:off + agent.dims[layout.HEAD[name]] - 1] > 0).sum())
        seen["logp_fused"].append(logprob.double().cpu().numpy())
        seen["logp_unfused"].append(lp_unfused.double().cpu().numpy())
        seen["logp_want"].append(lp_want)
        seen["value_fused"].append(value.double().cpu().numpy())
        seen["value_unfused"].append(v_unfused.flatten().double().cpu().numpy())
        seen["value_want"].append(v_want)

    stats = tr.evaluate(on_store=on_store)
    hook.remove()
    before = {k: p.detach().clone() for k, p in agent.named_parameters()}
    losses = tr.train()
    moved = {k: not torch.equal(before[k], p.detach()) for k, p in agent.named_parameters()}
    print("legal entries besides the no-op seen in the stores: "
          + ", ".join(f"{v} {TARGETS[k]}" for k, v in counts.items()))
    _run.update(tc=tc, stats=stats, ptr=tr.experience.ptr, losses=losses, moved=moved, obs_kept=obs_kept,
                counts=counts, seen={k: np.concatenate(v) for k, v in seen.items()})
    eng.close()
    return _run


def test_fused_evaluate_fills_the_batch_from_rows_with_legal_entities_in_all_three_target_heads():
    o = run()
    assert o["ptr"] == o["tc"].batch_size + 1 and o["stats"]["agent_SPS"] > 0
    assert all(v > 0 for v in o["counts"].values()), o["counts"]


def test_agent_forward_leaves_the_engines_obs_rows_unchanged():
    o = run()
    assert len(o["obs_kept"]) >= 4 and all(o["obs_kept"])


def test_stored_logprobs_and_values_stay_within_the_unfused_agents_error():
    s = run()["seen"]
    assert np.abs(s["value_want"]).max() > 0
    within("evaluate logprob", s["logp_fused"], s["logp_want"], s["logp_unfused"])
    within("evaluate value", s["value_fused"], s["value_want"], s["value_unfused"])


def test_fused_train_moves_every_player_path_parameter_with_finite_losses():
    o = run()
    for k in ("policy_loss", "value_loss", "entropy", "approx_kl", "clipfrac"):
        assert np.isfinite(o["losses"][k]), k
    player_params = {k: v for k, v in o["moved"].items() if k.startswith(PLAYER_LAYERS)}
    # player_encoder's agent_fc and my_agent_fc, the two projection layers, the three queries
    assert len(player_params) == 4 + 2 + 2 + 2 * 3 and all(player_params.values()), player_params
    assert all(o["moved"].values()), o["moved"]
