"""`baseline.BaselineAgent`, the start-kit Baseline assembled from this package's modules, without a
GPU: its `state_dict` has exactly the reference's parameter names and shapes (written out below from
baseline_policy.py:22-82 and the classes it builds), the unfused forward returns the four outputs of
the stand-ins' call convention on generated rows, its given-action logprob and entropy are the
reference's per-head `masked_fill(mask == 0, -1e9)` + `Categorical` expressions evaluated directly on
the reference's logits (embeddings, zero row, `matmul`), and every `fused_*` flag on host tensors is a
`HeadsError`, never a fallback. CPU only.

The mask rows follow tests/test_gpu_heads.py's `Case` (all illegal, all legal, first / last entry only,
an empty Buy head, random at 0.3), restated here because `Case` itself puts its tensors on the GPU."""

import numpy as np
import pytest
import torch

from nmmo_amd import layout
from nmmo_amd.baseline import DECODER_LAYERS, BaselineAgent
from nmmo_amd.heads import HeadsError
from tests.test_gpu_item import make_sets as make_item_sets
from tests.test_gpu_player import make_sets as make_entity_sets
from tests.test_tile_abi import sample_tiles

H, T = 256, 2048
# baseline_policy.py: TileEncoder :89-93, PlayerEncoder :120-121, ItemEncoder :151, InventoryEncoder :176,
# MarketEncoder :187, TaskEncoder :196, proj_fc :36, ActionDecoder :207-218, value_head :38
REFERENCE_STATE = {
    "tile_encoder.embedding.weight": (768, 32),
    "tile_encoder.tile_conv_1.weight": (32, 96, 3, 3), "tile_encoder.tile_conv_1.bias": (32,),
    "tile_encoder.tile_conv_2.weight": (8, 32, 3, 3), "tile_encoder.tile_conv_2.bias": (8,),
    "tile_encoder.tile_fc.weight": (H, 968), "tile_encoder.tile_fc.bias": (H,),
    "player_encoder.agent_fc.weight": (H, 35), "player_encoder.agent_fc.bias": (H,),
    "player_encoder.my_agent_fc.weight": (H, 35), "player_encoder.my_agent_fc.bias": (H,),
    "item_encoder.fc.weight": (H, 32), "item_encoder.fc.bias": (H,),
    "inventory_encoder.fc.weight": (H, 12 * H), "inventory_encoder.fc.bias": (H,),
    "market_encoder.fc.weight": (H, H), "market_encoder.fc.bias": (H,),
    "task_encoder.fc.weight": (H, T), "task_encoder.fc.bias": (H,),
    "proj_fc.weight": (H, 6 * H), "proj_fc.bias": (H,),
    "action_decoder.layers.attack_style.weight": (3, H), "action_decoder.layers.attack_style.bias": (3,),
    "action_decoder.layers.attack_target.weight": (H, H), "action_decoder.layers.attack_target.bias": (H,),
    "action_decoder.layers.market_buy.weight": (H, H), "action_decoder.layers.market_buy.bias": (H,),
    "action_decoder.layers.inventory_destroy.weight": (H, H), "action_decoder.layers.inventory_destroy.bias": (H,),
    "action_decoder.layers.inventory_give_item.weight": (H, H), "action_decoder.layers.inventory_give_item.bias": (H,),
    "action_decoder.layers.inventory_give_player.weight": (H, H), "action_decoder.layers.inventory_give_player.bias": (H,),
    "action_decoder.layers.gold_quantity.weight": (99, H), "action_decoder.layers.gold_quantity.bias": (99,),
    "action_decoder.layers.gold_target.weight": (H, H), "action_decoder.layers.gold_target.bias": (H,),
    "action_decoder.layers.move.weight": (5, H), "action_decoder.layers.move.bias": (5,),
    "action_decoder.layers.inventory_sell.weight": (H, H), "action_decoder.layers.inventory_sell.bias": (H,),
    "action_decoder.layers.inventory_price.weight": (99, H), "action_decoder.layers.inventory_price.bias": (99,),
    "action_decoder.layers.inventory_use.weight": (H, H), "action_decoder.layers.inventory_use.bias": (H,),
    "value_head.weight": (1, H), "value_head.bias": (1,),
}
BUY = layout.HEAD["Buy.MarketItem"]


def test_state_dict_has_exactly_the_references_names_and_shapes():
    sd = BaselineAgent().state_dict()
    assert list(sd) == list(REFERENCE_STATE)  # the reference's order too
    assert {k: tuple(v.shape) for k, v in sd.items()} == REFERENCE_STATE
    fused = BaselineAgent(fused_heads=True, fused_tile=True, fused_tile_conv2=True, fused_item=True, fused_player=True,
                          fused_decoder=True, seed=3, query_scale=0.5)
    assert list(fused.state_dict()) == list(sd)  # no flag changes a parameter
    fused.load_state_dict(sd, strict=True)
    assert [name for name, _ in DECODER_LAYERS] == [k.split(".")[2] for k in REFERENCE_STATE
                                                   if k.startswith("action_decoder") and k.endswith("weight")]


def test_defaults_are_the_references_and_unfused():
    a = BaselineAgent()
    assert (a.task_dim, a.query_scale, a.seed, a.draws) == (2048, 1.0, 0, 0)
    assert not (a.fused_heads or a.fused_decoder or a.tile_encoder.fused or a.tile_encoder.fused_conv2
                or a.item_encoder.fused or a.player_encoder.fused)
    assert a.dims == list(layout.ACTION_DIMS) and a.head_set == [-1, 0, 2, 1, 1, 0, -1, 0, -1, 1, -1, 1]
    assert a.pointer == [1, 2, 3, 4, 5, 7, 9, 11]


def make_rows(n, seed=0, task_dim=64):
    """n flat obs rows float32 from the existing generators, and the legal bits of their mask prefix."""
    rng = np.random.default_rng(seed)
    lay = layout.flat_layout(task_dim)
    obs = np.zeros((n, layout.obs_elems(task_dim)), dtype=np.float32)
    ents, ids = make_entity_sets(n, layout.PLAYER_N_OBS, rng, nan=False)
    sections = {"Entity": ents, "Inventory": make_item_sets(n, layout.INVENTORY_N_OBS, rng, nan=False),
                "Market": make_item_sets(n, layout.MARKET_N_OBS, rng, nan=False), "Tile": sample_tiles(n, rng),
                "Task": rng.standard_normal((n, task_dim)).astype(np.float32), "AgentId": ids.reshape(n, 1)}
    for name, x in sections.items():
        obs[:, lay[name].offset:lay[name].offset + int(np.prod(lay[name].shape))] = x.reshape(n, -1)
    dims = list(layout.ACTION_DIMS)
    off = np.cumsum([0] + dims)
    legal = rng.random((n, off[-1])) < 0.3
    legal[0], legal[1], legal[2], legal[3] = False, True, False, False
    for k in range(len(dims)):
        legal[2, off[k]] = True
        legal[3, off[k + 1] - 1] = True
    legal[4, off[BUY]:off[BUY + 1]] = False  # a living row whose Buy head alone is empty
    obs[:, :off[-1]] = np.where(legal, rng.choice([1.0, 0.5], legal.shape), 0.0)
    return torch.from_numpy(obs), legal


N = 6


@pytest.fixture(scope="module")
def run():
    torch.manual_seed(0)
    agent = BaselineAgent(64, 64)
    obs, legal = make_rows(N)
    kept = obs.clone()
    with torch.no_grad():
        sampled = agent(obs)
        given = agent(obs, action=sampled[0])
    return agent, obs, kept, legal, sampled, given


def test_unfused_forward_returns_the_four_outputs_and_leaves_the_rows_unchanged(run):
    agent, obs, kept, legal, sampled, given = run
    action, logprob, entropy, value = sampled
    assert tuple(action.shape) == (N, 12) and action.dtype == torch.int64
    assert tuple(logprob.shape) == (N,) and tuple(entropy.shape) == (N,) and tuple(value.shape) == (N, 1)
    assert all(torch.isfinite(t).all() for t in (logprob, entropy, value))
    assert torch.equal(obs, kept)
    off = np.cumsum([0] + agent.dims)
    a = action.numpy()
    for r in range(N):
        for k in range(12):
            if legal[r, off[k]:off[k + 1]].any():  # a sampled action is legal wherever one exists
                assert legal[r, off[k] + a[r, k]], (r, k)
    assert torch.equal(given[0], sampled[0]) and torch.equal(given[1], logprob) and torch.equal(given[2], entropy)
    assert agent.draws == 0  # the counter belongs to the philox paths


def test_given_action_logprob_and_entropy_are_the_references_expressions(run):
    agent, obs, _, legal, sampled, given = run
    action = sampled[0]
    with torch.no_grad():
        hidden = agent.encode_observations(obs)
        n = obs.shape[0]
        emb = {"Entity": agent.player_encoder.embed(agent.section(obs, "Entity").reshape(n, 100, 31)),
               "Inventory": agent.item_encoder.embed(agent.section(obs, "Inventory").reshape(n, 12, 16)),
               "Market": agent.item_encoder.embed(agent.section(obs, "Market").reshape(n, 1024, 16))}
        logp, ent = 0.0, 0.0
        off = np.cumsum([0] + agent.dims)
        for k, (name, s) in enumerate(DECODER_LAYERS):  # baseline_policy.py:222-230, then :245-262
            x = agent.action_decoder.layers[name](hidden)
            if s is not None:
                padded = torch.cat([emb[s], torch.zeros(n, 1, emb[s].shape[2])], 1)
                x = torch.matmul(padded, x.unsqueeze(-1)).squeeze(-1)
            x = x.masked_fill(obs[:, off[k]:off[k + 1]] == 0, -1e9)
            dist = torch.distributions.Categorical(logits=x)
            logp, ent = logp + dist.log_prob(action[:, k]), ent + dist.entropy()
        value = agent.value_head(hidden)
    # the mask prefix holds 0 where illegal, as the obs kernels write it: `== 0` is `not > 0`
    assert torch.equal(obs[:, :off[-1]] > 0, torch.from_numpy(legal))
    assert torch.equal(given[3], value)
    assert torch.equal(given[1], logp) and torch.equal(given[2], ent)
    assert float(ent.abs().max()) > 0


def test_encode_and_decode_compose_to_forward(run):
    agent, obs, _, _, sampled, given = run
    with torch.no_grad():
        hidden = agent.encode_observations(obs)
        assert tuple(hidden.shape) == (N, 64)
        out = agent.decode_actions(hidden, obs, sampled[0])
    for a, b in zip(out[1:], given[1:]):
        assert torch.equal(a, b)


def test_query_scale_scales_the_pointer_logits_only():
    torch.manual_seed(1)
    a, b = BaselineAgent(64, 64), BaselineAgent(64, 64, query_scale=0.125)
    b.load_state_dict(a.state_dict())
    obs, _ = make_rows(5, seed=2)
    with torch.no_grad():
        h = a.encode_observations(obs)
        out = [a.action_decoder.layers[name](h) for name, _ in DECODER_LAYERS]
        la = a.logits(out, {k: out[k] for k in a.pointer}, obs)
        lb = b.logits(out, {k: out[k] * 0.125 for k in b.pointer}, obs)
    off = np.cumsum([0] + a.dims)
    for k, s in enumerate(a.head_set):
        sl = slice(off[k], off[k + 1])
        assert torch.equal(lb[:, sl], la[:, sl] * 0.125 if s >= 0 else la[:, sl])  # a power of two: exact


@pytest.mark.parametrize("flags", [dict(fused_heads=True), dict(fused_tile=True),
                                   dict(fused_tile=True, fused_tile_conv2=True), dict(fused_item=True),
                                   dict(fused_player=True), dict(fused_decoder=True)])
def test_every_fused_flag_on_host_tensors_is_an_error(flags):
    agent = BaselineAgent(64, 64, **flags)
    obs, _ = make_rows(5, seed=1)
    with pytest.raises(HeadsError):
        with torch.no_grad():
            agent(obs)
    with pytest.raises(ValueError):
        BaselineAgent(64, 64, fused_tile_conv2=True)  # the second convolution extends the fused first one
