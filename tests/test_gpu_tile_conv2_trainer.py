"""The device evaluate/train loop with `TileMaskedAgent(fused_tile=True, fused_tile_conv2=True,
fused_heads=True)` on MI355X: the tile encoder with both convolutions in one kernel
(nmmo_amd/tile.py `tile_conv12`, SPEC.md §22) reading the engine's obs rows in place, in front of the
fused action heads. The shape and the yardsticks are test_gpu_tile_trainer.py's (C4, MAP_N=2, 2 envs,
batch_size 1024, batch_rows 16): every store is re-evaluated by an unfused float32 copy of the agent
on the GPU and by a float64 copy on the host, and the fused agent's error against the float64 values
stays within 4 x the unfused copy's (`within`)."""

import numpy as np
import pytest
import torch

from tests.conftest import gpu_available
from tests.test_gpu_heads import closed_form, within

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

_run = {}


def run():
    """One evaluate() (checked store by store) and one train() with the fused agent; cached."""
    if _run:
        return _run
    from nmmo_amd.config import Config
    from nmmo_amd.engine import NmmoEngine
    from nmmo_amd.trainer import DeviceTrainer, TileMaskedAgent, TrainConfig

    torch.manual_seed(0)
    cfg = Config.preset("C4", MAP_N=2, early_stop_agent_num=8)
    eng = NmmoEngine(cfg, 2, seed=5)
    eng.reset()
    agent = TileMaskedAgent(cfg.TASK_EMBED_DIM, fused_heads=True, seed=9, fused_tile=True, fused_tile_conv2=True).cuda()
    unfused = TileMaskedAgent(cfg.TASK_EMBED_DIM).cuda()
    unfused.load_state_dict(agent.state_dict())
    exact = TileMaskedAgent(cfg.TASK_EMBED_DIM)
    exact.load_state_dict(agent.state_dict())
    exact = exact.double()
    tc = TrainConfig(batch_size=1024, batch_rows=16, bptt_horizon=8, update_epochs=2, total_timesteps=4096)
    assert agent.tile_encoder.fused_conv2 and not unfused.tile_encoder.fused
    tr = DeviceTrainer(eng, agent, tc)
    total = sum(agent.dims)
    seen = {k: [] for k in ("logp_fused", "logp_unfused", "logp_want", "value_fused", "value_unfused", "value_want")}
    before_forward, obs_kept, tile_cols = [], [], []
    hook = agent.register_forward_pre_hook(lambda mod, args: before_forward.append(args[0].clone()))

    def on_store(o, r, d, mask, actions, logprob, value, env_id, step):
        obs_kept.append(torch.equal(o, before_forward[-1]))  # the forward wrote nothing into the obs rows
        with torch.no_grad():
            _, lp_unfused, _, v_unfused = unfused(o, action=actions.long())
            o64 = o.double().cpu()
            tick = o64[:, exact.o_tick:exact.o_tick + 1] / 1024.0
            h = exact.encoder(torch.cat([exact.tile_encoder(o64, exact.o_tile), tick], 1))
            lp_want = closed_form(exact.actor(h).numpy(), (o[:, :total] > 0).cpu().numpy(), agent.dims,
                                  actions.cpu().numpy())[0]
            v_want = exact.value(h).flatten().numpy()
        tile_cols.append(o[:, agent.o_tile:agent.o_tile + 675].cpu().numpy())
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
    finite = {k: bool(torch.isfinite(p).all()) for k, p in agent.named_parameters()}
    _run.update(tc=tc, stats=stats, ptr=tr.experience.ptr, losses=losses, moved=moved, finite=finite, obs_kept=obs_kept,
                tiles=np.concatenate(tile_cols), seen={k: np.concatenate(v) for k, v in seen.items()})
    eng.close()
    return _run


def test_fused_evaluate_fills_the_batch_from_real_tile_sections():
    o = run()
    assert o["ptr"] == o["tc"].batch_size + 1 and o["stats"]["agent_SPS"] > 0
    tiles = o["tiles"].reshape(-1, 225, 3)
    alive = tiles.any((1, 2))
    assert alive.sum() > 100  # rows of living agents, not only rows of agents not in the realm
    assert len(np.unique(tiles[alive][:, :, 2])) > 3  # several materials in view


def test_agent_forward_leaves_the_engines_obs_rows_unchanged():
    o = run()
    assert len(o["obs_kept"]) >= 4 and all(o["obs_kept"])


def test_stored_logprobs_and_values_stay_within_the_unfused_agents_error():
    s = run()["seen"]
    assert np.abs(s["value_want"]).max() > 0
    within("evaluate logprob", s["logp_fused"], s["logp_want"], s["logp_unfused"])
    within("evaluate value", s["value_fused"], s["value_want"], s["value_unfused"])


def test_fused_train_moves_every_tile_encoder_parameter_with_finite_losses():
    o = run()
    for k in ("policy_loss", "value_loss", "entropy", "approx_kl", "clipfrac"):
        assert np.isfinite(o["losses"][k]), k
    tile_params = {k: v for k, v in o["moved"].items() if k.startswith("tile_encoder.")}
    assert len(tile_params) == 7 and all(tile_params.values()), tile_params
    assert all(o["moved"].values()), o["moved"]
    assert all(o["finite"].values()), o["finite"]
