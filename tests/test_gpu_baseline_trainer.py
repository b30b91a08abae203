"""The device evaluate/train loop with `BaselineAgent`, every flag on (`fused_decoder=True` included), on
MI355X: the start-kit Baseline's twelve heads decoded from the engine's obs rows by one
`decoder.decoder_heads` call (SPEC.md §23) behind the fused encoders. The shape is
test_gpu_player_trainer.py's (C4, MAP_N=2, 2 envs, batch_size 1024, batch_rows 16, hidden 64, WARMUP
unstored ticks) with a random task embedding, so that the Task section is not all zero, and so is the
state edit, restated here: the players pairwise on one tile with 99 gold
each and past their immunity, each with one listed and one unlisted item. With it every pointer head
sees legal entries besides the no-op; the counts per head over the stores are asserted non-zero for all
eight pointer heads, because without that condition the test could not see a broken head.

At every store
  - a twin with the same `state_dict` and `fused_decoder=False`, the other flags equal (`item_logits`,
    `player_logits`, `cat`, `masked_heads`), re-evaluates the stored actions to the same logprob bits and,
    at the same `draws`, samples the same actions;
  - an unfused float32 copy on the GPU and a float64 copy on the host bound the whole agent: the fused
    agent's logprob and value errors against float64 are within 4 x the unfused copy's (`within`).
Then `train()`: finite losses, every parameter the forward uses moves, all twelve decoder layers and
`proj_fc` among them, and the forward leaves the engine's obs rows unchanged.

`query_scale` is 1 / sqrt(hidden), not the reference's 1.0: with freshly initialised weights a pointer
logit is a query times an embedding of raw entity columns in the hundreds, and at scale 1.0 the entity
heads are one-hot to the last bit, so their queries' gradients are exactly zero and "moves" could not
be asked of them. The stand-ins of `nmmo_amd/trainer.py` use the same scale for the same reason.

`inventory_encoder.fc` does not move and is asserted not to: the reference's forward never uses it
(baseline_policy.py:47-56 pools the item embeddings instead), and neither does `BaselineAgent`."""

import math

import numpy as np
import pytest
import torch

from tests.conftest import gpu_available
from tests.test_gpu_heads import closed_form, within

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

_run = {}
WARMUP = 8  # ticks before the stored batch: the players have moved and met NPCs
HIDDEN = 64
POINTER = ("Attack.Target", "Buy.MarketItem", "Destroy.InventoryItem", "Give.InventoryItem", "Give.Target",
           "GiveGold.Target", "Sell.InventoryItem", "Use.InventoryItem")
FUSED = dict(fused_heads=True, fused_tile=True, fused_tile_conv2=True, fused_item=True, fused_player=True)
UNUSED = ("inventory_encoder.fc.weight", "inventory_encoder.fc.bias")


def run():
    """One evaluate() (checked store by store) and one train() with the fused agent; cached."""
    if _run:
        return _run
    from nmmo_amd import abi, layout
    from nmmo_amd.baseline import DECODER_LAYERS, BaselineAgent
    from nmmo_amd.config import Config
    from nmmo_amd.engine import NmmoEngine
    from nmmo_amd.trainer import DeviceTrainer, TrainConfig
    from oracle.oracle import join_state, split_state

    torch.manual_seed(0)
    cfg = Config.preset("C4", MAP_N=2, early_stop_agent_num=8)
    # a Task section that is not all zero: task_encoder.fc.weight gets a gradient
    task = np.random.default_rng(3).standard_normal(cfg.TASK_EMBED_DIM).astype(np.float16)
    eng = NmmoEngine(cfg, 2, seed=5, task_embedding=task)
    eng.reset()
    scale = 1.0 / math.sqrt(HIDDEN)
    agent = BaselineAgent(cfg.TASK_EMBED_DIM, HIDDEN, seed=9, query_scale=scale, fused_decoder=True, **FUSED).cuda()
    twin = BaselineAgent(cfg.TASK_EMBED_DIM, HIDDEN, seed=9, query_scale=scale, fused_decoder=False, **FUSED).cuda()
    unfused = BaselineAgent(cfg.TASK_EMBED_DIM, HIDDEN, query_scale=scale).cuda()
    exact = BaselineAgent(cfg.TASK_EMBED_DIM, HIDDEN, query_scale=scale)
    for other in (twin, unfused, exact):
        other.load_state_dict(agent.state_dict())
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
    before_forward, obs_kept, twin_bits, twin_samples = [], [], [], []
    counts = {name: 0 for name in POINTER}
    hook = agent.register_forward_pre_hook(lambda mod, args: before_forward.append(args[0].clone()))

    def on_store(o, r, d, mask, actions, logprob, value, env_id, step):
        obs_kept.append(torch.equal(o, before_forward[-1]))  # the forward wrote nothing into the obs rows
        with torch.no_grad():
            twin.draws = agent.draws - 1  # the draw the stored actions came from
            a_twin, _, _, _ = twin(o)
            _, lp_twin, _, _ = twin(o, action=actions)
            twin_samples.append(a_twin.dtype == actions.dtype and torch.equal(a_twin, actions))
            twin_bits.append(torch.equal(lp_twin.view(torch.int32), logprob.view(torch.int32)))
            _, lp_unfused, _, v_unfused = unfused(o, action=actions.long())
            o64 = o.double().cpu()
            h, emb = exact._encode(o64)
            out = [exact.action_decoder.layers[name](h) for name, _ in DECODER_LAYERS]
            logits = exact.logits(out, {k: out[k] * scale for k in exact.pointer}, o64, emb)
            lp_want = closed_form(logits.numpy(), (o[:, :total] > 0).cpu().numpy(), agent.dims, actions.cpu().numpy())[0]
            v_want = exact.value_head(h).flatten().numpy()
        for name in POINTER:
            k = layout.HEAD[name]
            counts[name] += int((o[:, agent.mask_off[k]:agent.mask_off[k + 1] - 1] > 0).sum())
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
    print("legal entries besides the no-op seen in the stores: " + ", ".join(f"{v} {k}" for k, v in counts.items()))
    _run.update(tc=tc, stats=stats, ptr=tr.experience.ptr, losses=losses, moved=moved, obs_kept=obs_kept,
                counts=counts, twin_bits=twin_bits, twin_samples=twin_samples,
                seen={k: np.concatenate(v) for k, v in seen.items()})
    eng.close()
    return _run


def test_fused_evaluate_fills_the_batch_from_rows_with_legal_entries_in_all_eight_pointer_heads():
    o = run()
    assert o["ptr"] == o["tc"].batch_size + 1 and o["stats"]["agent_SPS"] > 0
    assert len(o["counts"]) == 8 and all(v > 0 for v in o["counts"].values()), o["counts"]


def test_agent_forward_leaves_the_engines_obs_rows_unchanged():
    o = run()
    assert len(o["obs_kept"]) >= 4 and all(o["obs_kept"])


def test_the_composed_twin_gives_the_same_logprob_bits_and_the_same_samples():
    o = run()
    assert len(o["twin_bits"]) >= 4 and all(o["twin_bits"]), o["twin_bits"]
    assert all(o["twin_samples"]), o["twin_samples"]


def test_stored_logprobs_and_values_stay_within_the_unfused_agents_error():
    s = run()["seen"]
    assert np.abs(s["value_want"]).max() > 0
    within("evaluate logprob", s["logp_fused"], s["logp_want"], s["logp_unfused"])
    within("evaluate value", s["value_fused"], s["value_want"], s["value_unfused"])


def test_fused_train_moves_every_parameter_the_forward_uses_with_finite_losses():
    from nmmo_amd.baseline import DECODER_LAYERS

    o = run()
    for k in ("policy_loss", "value_loss", "entropy", "approx_kl", "clipfrac"):
        assert np.isfinite(o["losses"][k]), k
    moved = o["moved"]
    for name, _ in DECODER_LAYERS:  # all twelve decoder layers
        assert moved[f"action_decoder.layers.{name}.weight"] and moved[f"action_decoder.layers.{name}.bias"], name
    assert moved["proj_fc.weight"] and moved["proj_fc.bias"]
    assert not [k for k, v in moved.items() if not v and k not in UNUSED]
    assert not any(moved[k] for k in UNUSED)  # as in the reference: built, loaded, never used
    assert len(moved) == 47
