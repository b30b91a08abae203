"""The device evaluate/train loop with `reduced.ReducedAgent`, every flag on, on MI355X: the takeru
policy's pointer heads from `embed.embed_logits` over the engine's obs rows (SPEC.md §25) behind the fused
encoders. The shape and the state edit are test_gpu_baseline_trainer.py's, restated here (C4, MAP_N=2,
2 envs, batch_size 1024, batch_rows 16, hidden = input = 64, WARMUP unstored ticks, a random task
embedding; the players pairwise on one tile with 99 gold each and past their immunity, each with one
listed and one unlisted item), and so is `query_scale` = 1 / sqrt(hidden), for the reason given there.
The legal entries besides the no-op are counted per head over the stores and asserted non-zero for
all eight pointer heads.

At every store an unfused float32 copy on the GPU and a float64 copy on the host bound the whole agent:
the fused agent's logprob and value errors against float64 are within 4 x the unfused copy's
(`within`), and the forward leaves the engine's obs rows unchanged. Then `train()`: finite losses,
every parameter moves (this policy's forward uses all 49, `inventory_encoder.fc` included), and of the
three embedding tables only rows that were indexed move: the entity table's rows 256.. never do
(the clip comes after the offset). `RecurrentReducedAgent` runs one evaluate() + train() with
`fused_lstm=True`, and `run_policy(..., greedy=True)` gives the same actions and rewards on two runs."""

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
SCALE = 1.0 / math.sqrt(HIDDEN)
POINTER = ("Attack.Target", "Buy.MarketItem", "Destroy.InventoryItem", "Give.InventoryItem", "Give.Target",
           "GiveGold.Target", "Sell.InventoryItem", "Use.InventoryItem")
FUSED = dict(fused_heads=True, fused_tile=True, fused_tile_conv2=True, fused_item=True, fused_player=True)
TABLES = ("tile_encoder.embedding.weight", "player_encoder.embedding.weight", "item_encoder.embedding.weight")


def make_engine(agent=None, warmup=0):
    """The engine of test_gpu_baseline_trainer.py: `warmup` ticks of the agent's own rollout, then its
    state edit."""
    from nmmo_amd import abi
    from nmmo_amd.config import Config
    from nmmo_amd.engine import NmmoEngine
    from oracle.oracle import join_state, split_state

    cfg = Config.preset("C4", MAP_N=2, early_stop_agent_num=8)
    # a Task section that is not all zero: task_encoder.fc.weight gets a gradient
    task = np.random.default_rng(3).standard_normal(cfg.TASK_EMBED_DIM).astype(np.float16)
    eng = NmmoEngine(cfg, 2, seed=5, task_embedding=task)
    eng.reset()
    n_rows = eng.n_envs * eng.P
    for _ in range(warmup):
        with torch.no_grad():
            actions = agent(eng.obs.view(n_rows, eng.obs_elems))[0]
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
    return eng, cfg


def task_dim():
    from nmmo_amd.config import Config

    return Config.preset("C4", MAP_N=2, early_stop_agent_num=8).TASK_EMBED_DIM


def indexed_rows(agent, obs_list):
    """{table: bool [rows]} of the table rows the forward reads on the stored obs rows."""
    from nmmo_amd import embed, layout, tile

    used = {k: torch.zeros(dict(agent.named_parameters())[k].shape[0], dtype=torch.bool, device="cuda") for k in TABLES}
    for o in obs_list:
        n = o.shape[0]
        mat = tile.tile_indices(o[:, agent.o_tile:agent.o_tile + tile.ROW])[:, :, 2]
        used[TABLES[0]][mat.flatten()] = True
        ents = agent.section(o, "Entity").reshape(n, layout.PLAYER_N_OBS, 31)
        used[TABLES[1]][embed.embed_features_ref(embed.ENTITY, ents)[0].flatten()] = True
        for name, rows in (("Inventory", layout.INVENTORY_N_OBS), ("Market", layout.MARKET_N_OBS)):
            items = agent.section(o, name).reshape(n, rows, 16)
            used[TABLES[2]][embed.embed_features_ref(embed.ITEM, items)[0].flatten()] = True
    return used


def run():
    """One evaluate() (checked store by store) and one train() with the fused agent; cached."""
    if _run:
        return _run
    from nmmo_amd import layout
    from nmmo_amd.baseline import DECODER_LAYERS
    from nmmo_amd.reduced import ReducedAgent
    from nmmo_amd.trainer import DeviceTrainer, TrainConfig

    torch.manual_seed(0)
    T = task_dim()
    agent = ReducedAgent(T, HIDDEN, HIDDEN, seed=9, query_scale=SCALE, **FUSED).cuda()
    unfused = ReducedAgent(T, HIDDEN, HIDDEN, query_scale=SCALE).cuda()
    exact = ReducedAgent(T, HIDDEN, HIDDEN, query_scale=SCALE)
    for other in (unfused, exact):
        other.load_state_dict(agent.state_dict(), strict=True)
    exact = exact.double()
    eng, cfg = make_engine(agent, WARMUP)
    tc = TrainConfig(batch_size=1024, batch_rows=16, bptt_horizon=8, update_epochs=2, total_timesteps=4096)
    tr = DeviceTrainer(eng, agent, tc)
    total = sum(agent.dims)
    seen = {k: [] for k in ("logp_fused", "logp_unfused", "logp_want", "value_fused", "value_unfused", "value_want")}
    before_forward, obs_kept, stored = [], [], []
    counts = {name: 0 for name in POINTER}
    hook = agent.register_forward_pre_hook(lambda mod, args: before_forward.append(args[0].clone()))

    def on_store(o, r, d, mask, actions, logprob, value, env_id, step):
        obs_kept.append(torch.equal(o, before_forward[-1]))  # the forward wrote nothing into the obs rows
        stored.append(o.clone())
        with torch.no_grad():
            _, lp_unfused, _, v_unfused = unfused(o, action=actions.long())
            o64 = o.double().cpu()
            h, emb = exact._encode(o64)
            out = [exact.action_decoder.layers[name](h) for name, _ in DECODER_LAYERS]
            logits = exact.logits(out, {k: out[k] * SCALE for k in exact.pointer}, o64, emb)
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
    used = indexed_rows(agent, stored)
    before = {k: p.detach().clone() for k, p in agent.named_parameters()}
    losses = tr.train()
    after = dict(agent.named_parameters())
    moved = {k: not torch.equal(before[k], p.detach()) for k, p in after.items()}
    rows_moved = {k: (before[k] != after[k].detach()).any(1) for k in TABLES}
    print("legal entries besides the no-op seen in the stores: " + ", ".join(f"{v} {k}" for k, v in counts.items()))
    _run.update(tc=tc, stats=stats, ptr=tr.experience.ptr, losses=losses, moved=moved, obs_kept=obs_kept, counts=counts,
                used=used, rows_moved=rows_moved, seen={k: np.concatenate(v) for k, v in seen.items()})
    eng.close()
    return _run


def test_fused_evaluate_fills_the_batch_from_rows_with_legal_entries_in_all_eight_pointer_heads():
    o = run()
    assert o["ptr"] == o["tc"].batch_size + 1 and o["stats"]["agent_SPS"] > 0
    assert len(o["counts"]) == 8 and all(v > 0 for v in o["counts"].values()), o["counts"]


def test_agent_forward_leaves_the_engines_obs_rows_unchanged():
    o = run()
    assert len(o["obs_kept"]) >= 4 and all(o["obs_kept"])


def test_stored_logprobs_and_values_stay_within_the_unfused_agents_error():
    s = run()["seen"]
    assert np.abs(s["value_want"]).max() > 0
    within("evaluate logprob", s["logp_fused"], s["logp_want"], s["logp_unfused"])
    within("evaluate value", s["value_fused"], s["value_want"], s["value_unfused"])


def test_fused_train_moves_every_parameter_and_only_the_indexed_table_rows():
    o = run()
    for k in ("policy_loss", "value_loss", "entropy", "approx_kl", "clipfrac"):
        assert np.isfinite(o["losses"][k]), k
    moved = o["moved"]
    assert len(moved) == 49 and not [k for k, v in moved.items() if not v]
    for k in TABLES:
        used, rows = o["used"][k], o["rows_moved"][k]
        print(f"{k}: {int(used.sum())} rows indexed, {int(rows.sum())} moved")
        assert bool(rows.any()) and not bool((rows & ~used).any()), k
    assert not bool(o["rows_moved"][TABLES[1]][256:].any())


def test_the_recurrent_agent_evaluates_and_trains_with_the_fused_lstm():
    from nmmo_amd.reduced import RecurrentReducedAgent
    from nmmo_amd.trainer import DeviceTrainer, TrainConfig

    torch.manual_seed(1)
    agent = RecurrentReducedAgent(task_dim(), HIDDEN, input_size=HIDDEN, fused_lstm=True, seed=9, query_scale=SCALE,
                                  **FUSED).cuda()
    eng, cfg = make_engine()
    tc = TrainConfig(batch_size=1024, batch_rows=16, bptt_horizon=8, update_epochs=1, total_timesteps=4096)
    tr = DeviceTrainer(eng, agent, tc)
    n = eng.n_envs * eng.P
    assert tuple(tr.next_lstm_state[0].shape) == (1, n, HIDDEN)
    tr.evaluate()
    assert tr.experience.ptr == tc.batch_size + 1 and float(tr.next_lstm_state[0].abs().max()) > 0
    before = {k: p.detach().clone() for k, p in agent.named_parameters()}
    losses = tr.train()
    eng.close()
    for k in ("policy_loss", "value_loss", "entropy", "approx_kl", "clipfrac"):
        assert np.isfinite(losses[k]), k
    moved = {k: not torch.equal(before[k], p.detach()) for k, p in agent.named_parameters()}
    want = [k for k in moved if k.startswith("recurrent.")] + ["policy.proj_fc.weight", "policy.proj_fc.bias",
                                                               "policy.player_encoder.embedding.weight"]
    assert len(want) == 7 and all(moved[k] for k in want), [k for k in want if not moved[k]]


def test_run_policy_is_deterministic_when_greedy():
    from nmmo_amd.reduced import ReducedAgent
    from nmmo_amd.rollout import run_policy

    torch.manual_seed(2)
    agent = ReducedAgent(task_dim(), HIDDEN, HIDDEN, seed=9, query_scale=SCALE, **FUSED).cuda()
    runs = []
    for _ in range(2):
        eng, cfg = make_engine()
        acts = []
        out = run_policy(eng, agent, 8, greedy=True, on_step=lambda o, a, lp, v: acts.append(a.clone()))
        eng.close()
        assert out["steps"] == 8 and len(acts) == 8 and out["agent_steps"] > 0 and agent.draws == 0
        runs.append((torch.stack(acts), out["reward_sum"]))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert len(torch.unique(runs[0][0])) > 1
