"""The device evaluate/train loop with `ItemMaskedAgent(fused_item=True, fused_heads=True)` on
MI355X: the item-encoder kernels (nmmo_amd/item.py, SPEC.md §20) reading the Inventory and Market
sections of the engine's obs rows in place, their logits in front of the fused action heads. The
shape is test_gpu_tile_trainer.py's (C4, MAP_N=2, 2 envs, batch_size 1024, batch_rows 16). Every
store is re-evaluated by an unfused float32 copy of the agent on the GPU (embeddings, zero row,
matmul: the reference's way) and by a float64 copy on the host (its logits through
test_gpu_heads.py's float64 closed form of §15), and the fused agent's error against the float64
values stays within 4 x the unfused copy's (`within`).

Agents start with empty inventories, nothing is listed at reset and nobody has gold. In a rollout
of this agent from the reset the first items appear by tick 4 and the first listings by tick 8, but
no Buy entry besides the no-op is legal within 96 ticks: nobody can pay. A head whose only legal
entry is the no-op gives its query no gradient, fused or not. So the test first steps the agent's
own rollout for WARMUP ticks, unstored, then gives every player 99 gold (get_state / set_state), so
that the stored rows hold items, listings and legal Buy entries and every one of the five queries
takes part. The counts the stores saw (`items`, `listings`, `buys`) are asserted to be non-zero:
if one of them were zero, the Market path would rest on test_gpu_item.py alone."""

import numpy as np
import pytest
import torch

from tests.conftest import gpu_available
from tests.test_gpu_heads import closed_form, within

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

_run = {}
WARMUP = 16  # ticks before the stored batch: items by tick 4, listings by tick 8 (see above)
ITEM_LAYERS = ("item_encoder.", "inventory.", "market.", "queries.")


def run():
    """One evaluate() (checked store by store) and one train() with the fused agent; cached."""
    if _run:
        return _run
    from nmmo_amd import abi, layout
    from nmmo_amd.config import Config
    from nmmo_amd.engine import NmmoEngine
    from nmmo_amd.trainer import DeviceTrainer, ItemMaskedAgent, TrainConfig
    from oracle.oracle import join_state, split_state

    torch.manual_seed(0)
    cfg = Config.preset("C4", MAP_N=2, early_stop_agent_num=8)
    eng = NmmoEngine(cfg, 2, seed=5)
    eng.reset()
    agent = ItemMaskedAgent(cfg.TASK_EMBED_DIM, fused_heads=True, seed=9, fused_item=True).cuda()
    unfused = ItemMaskedAgent(cfg.TASK_EMBED_DIM).cuda()
    unfused.load_state_dict(agent.state_dict())
    exact = ItemMaskedAgent(cfg.TASK_EMBED_DIM)
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
    state["ent"][:, abi.F["gold"], :eng.P] = 99  # everyone can pay: Buy entries become legal
    eng.set_state(join_state(state))
    eng.observe()
    before_forward, obs_kept, items, listings, buys = [], [], 0, 0, 0
    hook = agent.register_forward_pre_hook(lambda mod, args: before_forward.append(args[0].clone()))

    def on_store(o, r, d, mask, actions, logprob, value, env_id, step):
        nonlocal items, listings, buys
        obs_kept.append(torch.equal(o, before_forward[-1]))  # the forward wrote nothing into the obs rows
        with torch.no_grad():
            _, lp_unfused, _, v_unfused = unfused(o, action=actions.long())
            o64 = o.double().cpu()
            h, inv_emb, mk_emb = exact.hidden(o64)
            lp_want = closed_form(exact.logits(h, o64, inv_emb, mk_emb).numpy(), (o[:, :total] > 0).cpu().numpy(),
                                  agent.dims, actions.cpu().numpy())[0]
            v_want = exact.value(h).flatten().numpy()
        inv, mk = agent.item_sets(o)
        items += int((inv[:, ::16] != 0).sum())
        listings += int((mk[:, ::16] != 0).sum())
        buy = agent.mask_off[layout.HEAD["Buy.MarketItem"]]
        buys += int((o[:, buy:buy + layout.MARKET_N_OBS] > 0).sum())
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
    print(f"item rows seen in the stores: {items} inventory items, {listings} listings, {buys} legal Buy entries")
    _run.update(tc=tc, stats=stats, ptr=tr.experience.ptr, losses=losses, moved=moved, obs_kept=obs_kept,
                items=items, listings=listings, buys=buys, seen={k: np.concatenate(v) for k, v in seen.items()})
    eng.close()
    return _run


def test_fused_evaluate_fills_the_batch_from_rows_with_items_listings_and_legal_buys():
    o = run()
    assert o["ptr"] == o["tc"].batch_size + 1 and o["stats"]["agent_SPS"] > 0
    assert o["items"] > 0 and o["listings"] > 0 and o["buys"] > 0, (o["items"], o["listings"], o["buys"])


def test_agent_forward_leaves_the_engines_obs_rows_unchanged():
    o = run()
    assert len(o["obs_kept"]) >= 4 and all(o["obs_kept"])


def test_stored_logprobs_and_values_stay_within_the_unfused_agents_error():
    s = run()["seen"]
    assert np.abs(s["value_want"]).max() > 0
    within("evaluate logprob", s["logp_fused"], s["logp_want"], s["logp_unfused"])
    within("evaluate value", s["value_fused"], s["value_want"], s["value_unfused"])


def test_fused_train_moves_every_item_path_parameter_with_finite_losses():
    o = run()
    for k in ("policy_loss", "value_loss", "entropy", "approx_kl", "clipfrac"):
        assert np.isfinite(o["losses"][k]), k
    item_params = {k: v for k, v in o["moved"].items() if k.startswith(ITEM_LAYERS)}
    assert len(item_params) == 2 + 2 + 2 + 2 * 5 and all(item_params.values()), item_params
    assert all(o["moved"].values()), o["moved"]
