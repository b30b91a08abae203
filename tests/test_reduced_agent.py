"""`reduced.ReducedAgent` and `reduced.RecurrentReducedAgent`, the takeru policy assembled from this
package's modules, without a GPU: the `state_dict` has exactly the reference's parameter names and
shapes (written out below from takeru/policy.py:24-37 and the constructors of the classes it builds),
a dict of random tensors with those names and shapes loads with `strict=True` under every flag
combination, the unfused forward in float64 equals this file's own restatement of the reference's
forward (gather, cat, fc, zero row, matmul, `masked_fill(mask == 0, -1e9)`, `Categorical`) on
generated rows with legal entries in all eight pointer heads, and every `fused_*` flag on host tensors
is a `HeadsError`, never a fallback. CPU only."""

import itertools

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from nmmo_amd import layout
from nmmo_amd.baseline import DECODER_LAYERS
from nmmo_amd.heads import HeadsError
from nmmo_amd.reduced import RecurrentReducedAgent, ReducedAgent, ReducedTileEncoder
from tests.test_baseline_agent import make_rows

FLAGS = ("fused_tile", "fused_tile_conv2", "fused_player", "fused_item", "fused_heads")
POINTER_SETS = {"attack_target": "Entity", "market_buy": "Market", "inventory_destroy": "Inventory",
                "inventory_give_item": "Inventory", "inventory_give_player": "Entity", "gold_target": "Entity",
                "inventory_sell": "Inventory", "inventory_use": "Inventory"}


def reference_state(I=256, H=256, T=2048):
    """takeru/policy.py: ReducedTileEncoder :88-92, ReducedPlayerEncoder :167-171, ReducedItemEncoder :219-221,
    InventoryEncoder :264, MarketEncoder :275, TaskEncoder :284, proj_fc :35, ReducedActionDecoder :308-325,
    value_head :37. The offsets and scales are plain attributes there, not buffers."""
    state = {
        "tile_encoder.embedding.weight": (256, 32),
        "tile_encoder.tile_conv_1.weight": (16, 32, 3, 3), "tile_encoder.tile_conv_1.bias": (16,),
        "tile_encoder.tile_conv_2.weight": (8, 16, 3, 3), "tile_encoder.tile_conv_2.bias": (8,),
        "tile_encoder.tile_fc.weight": (I, 8 * 11 * 11), "tile_encoder.tile_fc.bias": (I,),
        "player_encoder.embedding.weight": (4 * 256, 32),
        "player_encoder.agent_fc.weight": (H, 4 * 32 + 27), "player_encoder.agent_fc.bias": (H,),
        "player_encoder.my_agent_fc.weight": (I, 4 * 32 + 27), "player_encoder.my_agent_fc.bias": (I,),
        "item_encoder.embedding.weight": (256, 32),
        "item_encoder.fc.weight": (H, 2 * 32 + 12), "item_encoder.fc.bias": (H,),
        "inventory_encoder.fc.weight": (I, 12 * H), "inventory_encoder.fc.bias": (I,),
        "market_encoder.fc.weight": (I, H), "market_encoder.fc.bias": (I,),
        "task_encoder.fc.weight": (I, T), "task_encoder.fc.bias": (I,),
        "proj_fc.weight": (H, 5 * I), "proj_fc.bias": (H,),
    }
    for name, n in (("attack_style", 3), ("attack_target", H), ("market_buy", H), ("inventory_destroy", H),
                    ("inventory_give_item", H), ("inventory_give_player", H), ("gold_quantity", 99), ("gold_target", H),
                    ("move", 5), ("inventory_sell", H), ("inventory_price", 99), ("inventory_use", H)):
        state[f"action_decoder.layers.{name}.weight"] = (n, H)
        state[f"action_decoder.layers.{name}.bias"] = (n,)
    state["value_head.weight"], state["value_head.bias"] = (1, H), (1,)
    return state


def combos():
    for bits in itertools.product((False, True), repeat=len(FLAGS)):
        flags = dict(zip(FLAGS, bits))
        if flags["fused_tile_conv2"] and not flags["fused_tile"]:
            continue  # the second convolution extends the fused first one: a ValueError, checked below
        yield flags


def test_state_dict_has_exactly_the_references_names_and_shapes():
    sd = ReducedAgent().state_dict()
    want = reference_state()
    assert list(sd) == list(want) and len(want) == 49  # the reference's order too
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert [name for name, _ in DECODER_LAYERS] == [k.split(".")[2] for k in want
                                                   if k.startswith("action_decoder") and k.endswith("weight")]
    a = ReducedAgent()
    assert (a.task_dim, a.query_scale, a.seed, a.draws) == (2048, 1.0, 0, 0)
    assert not (a.fused_heads or a.fused_decoder or a.tile_encoder.fused or a.tile_encoder.fused_conv2
                or a.item_encoder.fused or a.player_encoder.fused)
    assert a.dims == list(layout.ACTION_DIMS) and a.pointer == [1, 2, 3, 4, 5, 7, 9, 11]


def test_a_random_state_dict_of_the_references_shapes_loads_strictly_under_every_flag_combination():
    I, H, T = 48, 64, 32
    want = reference_state(I, H, T)
    g = torch.Generator().manual_seed(0)
    sd = {k: torch.randn(shape, generator=g) for k, shape in want.items()}
    lstm = {f"recurrent.{p}_l0": torch.randn(shape, generator=g)
            for p, shape in (("weight_ih", (4 * H, H)), ("weight_hh", (4 * H, H)), ("bias_ih", (4 * H,)), ("bias_hh", (4 * H,)))}
    rsd = {**{"policy." + k: v for k, v in sd.items()}, **lstm}
    n = 0
    for flags in combos():
        a = ReducedAgent(T, I, H, seed=3, query_scale=0.5, **flags)
        a.load_state_dict(sd, strict=True)
        assert all(torch.equal(v, sd[k]) for k, v in a.state_dict().items()) and list(a.state_dict()) == list(sd)
        for fused_lstm in (False, True):
            r = RecurrentReducedAgent(T, H, input_size=I, fused_lstm=fused_lstm, **flags)
            r.load_state_dict(rsd, strict=True)
            assert list(r.state_dict()) == list(rsd) and r.lstm is r.recurrent and r.recurrent.num_layers == 1
            assert isinstance(r.policy, ReducedAgent)
        n += 1
    assert n == 24
    with pytest.raises(ValueError):
        ReducedAgent(T, I, H, fused_tile_conv2=True)
    with pytest.raises(ValueError):
        ReducedTileEncoder(I, fused_conv2=True)


# ---------------------------------------------------------------- the reference's forward, restated
ENTITY_DISCRETE, ITEM_DISCRETE = [0, 1, 8, 10], [1, 14]
ENTITY_CONT = [2, 3, 4, 5, 6, 7, 9] + list(range(11, 31))
ENTITY_SCALE = [256, 256, 100, 1024, 3, 50, 1024, 100, 100, 100, 100] + [10, 100] * 7 + [100, 10]
ITEM_CONT = [3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15]
ITEM_SCALE = [10, 10, 10, 100, 100, 100, 40, 40, 40, 100, 100, 100]


def reference_forward(sd, obs, lay, T, action, scale):
    """takeru/policy.py:39-64, 94-112, 173-207, 243-258, 266-287, 351-405 on the flat rows, with the
    start kit's per-head `masked_fill` + `Categorical` behind it; `sd` holds the parameters."""
    n = obs.shape[0]
    dt = obs.dtype

    def lin(name, x):
        return F.linear(x, sd[name + ".weight"], sd[name + ".bias"])

    def sec(name):
        s = lay[name]
        return obs[:, s.offset:s.offset + int(np.prod(s.shape))].reshape(n, *s.shape)

    def embed_rows(x, table, discrete, offset, cont, scales):
        d = x[:, :, discrete] + torch.tensor(offset, dtype=dt)
        d = sd[table][d.long().clip(0, 255)]
        d = d.view(n, x.shape[1], -1)
        return torch.cat([d, x[:, :, cont] / torch.tensor(scales, dtype=dt)], -1)

    t = sd["tile_encoder.embedding.weight"][sec("Tile")[:, :, 2].long().clip(0, 255)]  # [n, 225, 32]
    t = t.transpose(1, 2).reshape(n, 32, 15, 15)
    t = F.relu(F.conv2d(t, sd["tile_encoder.tile_conv_1.weight"], sd["tile_encoder.tile_conv_1.bias"]))
    t = F.relu(F.conv2d(t, sd["tile_encoder.tile_conv_2.weight"], sd["tile_encoder.tile_conv_2.bias"]))
    tile = F.relu(lin("tile_encoder.tile_fc", t.reshape(n, -1)))

    agents, my_id = sec("Entity"), sec("AgentId")[:, 0]
    ids = agents[:, :, 0]
    mask = ((ids == my_id.unsqueeze(1)) & (ids != 0)).int()
    row = torch.where(mask.any(1), mask.argmax(1), torch.zeros_like(mask.sum(1)))
    feat = embed_rows(agents, "player_encoder.embedding.weight", ENTITY_DISCRETE, [0, 256, 512, 768], ENTITY_CONT,
                      ENTITY_SCALE)
    my_agent = F.relu(lin("player_encoder.my_agent_fc", feat[torch.arange(n), row]))
    emb = {"Entity": lin("player_encoder.agent_fc", feat)}
    for name in ("Inventory", "Market"):
        emb[name] = lin("item_encoder.fc", embed_rows(sec(name), "item_encoder.embedding.weight", ITEM_DISCRETE, [2, 0],
                                                      ITEM_CONT, ITEM_SCALE))
    inventory = lin("inventory_encoder.fc", emb["Inventory"].reshape(n, -1))
    market = lin("market_encoder.fc", emb["Market"]).mean(-2)
    task = lin("task_encoder.fc", sec("Task").reshape(n, T))
    hidden = lin("proj_fc", torch.cat([tile, my_agent, inventory, market, task], -1))

    off = np.cumsum([0] + list(layout.ACTION_DIMS))
    logp, ent = 0.0, 0.0
    for k, (name, _) in enumerate(DECODER_LAYERS):
        x = lin(f"action_decoder.layers.{name}", hidden)
        if name in POINTER_SETS:
            e = emb[POINTER_SETS[name]]
            e = torch.cat([e, torch.zeros(n, 1, e.shape[2], dtype=dt)], 1)
            x = torch.matmul(e, (x * scale).unsqueeze(-1)).squeeze(-1)
        x = x.masked_fill(obs[:, off[k]:off[k + 1]] == 0, -1e9)
        dist = torch.distributions.Categorical(logits=x)
        logp, ent = logp + dist.log_prob(action[:, k]), ent + dist.entropy()
    return hidden, logp, ent, lin("value_head", hidden)


N, I, H, T = 6, 48, 64, 64


@pytest.fixture(scope="module")
def run():
    torch.manual_seed(0)
    agent = ReducedAgent(T, I, H, query_scale=0.125).double()
    obs, legal = make_rows(N, task_dim=T)
    obs = obs.double()
    kept = obs.clone()
    with torch.no_grad():
        sampled = agent(obs)
        given = agent(obs, action=sampled[0])
    return agent, obs, kept, legal, sampled, given


def test_the_rows_have_legal_entries_in_all_eight_pointer_heads(run):
    agent, obs, _, legal, _, _ = run
    off = np.cumsum([0] + agent.dims)
    for k in agent.pointer:
        assert legal[:, off[k]:off[k + 1] - 1].any(), k
    # and discrete columns on both sides of the clip: the generators' npc_type and item type classes
    ents = agent.section(obs, "Entity").reshape(N, 100, 31)
    assert float(ents[:, :, 0].min()) < 0 and float(ents[:, :, 0].max()) > 255


def test_unfused_forward_returns_the_four_outputs_and_leaves_the_rows_unchanged(run):
    agent, obs, kept, legal, sampled, given = run
    action, logprob, entropy, value = sampled
    assert tuple(action.shape) == (N, 12) and action.dtype == torch.int64
    assert tuple(logprob.shape) == (N,) and tuple(entropy.shape) == (N,) and tuple(value.shape) == (N, 1)
    assert all(torch.isfinite(t).all() for t in (logprob, entropy, value))
    assert torch.equal(obs, kept) and agent.draws == 0
    assert torch.equal(given[0], action) and torch.equal(given[1], logprob) and torch.equal(given[2], entropy)
    greedy = agent(obs, greedy=True)
    off = np.cumsum([0] + agent.dims)
    for r in range(N):
        for k in range(12):
            if legal[r, off[k]:off[k + 1]].any():  # a sampled or selected action is legal wherever one exists
                assert legal[r, off[k] + int(action[r, k])] and legal[r, off[k] + int(greedy[0][r, k])], (r, k)
    with pytest.raises(ValueError):
        agent(obs, action=action, greedy=True)


def test_the_float64_forward_is_the_references(run):
    agent, obs, _, _, sampled, given = run
    lay = layout.flat_layout(T)
    with torch.no_grad():
        hidden, logp, ent, value = reference_forward(agent.state_dict(), obs, lay, T, sampled[0], 0.125)
        got_hidden = agent.encode_observations(obs)
    # float64 rounding: the two chains add the same terms, torch choosing the order in each
    for name, got, want in (("hidden", got_hidden, hidden), ("logprob", given[1], logp), ("entropy", given[2], ent),
                            ("value", given[3], value)):
        err, size = float((got - want).abs().max()), float(want.abs().max())
        print(f"{name}: max |got - want| {err:.3e} of {size:.3e}")
        assert err <= 1e-9 * max(size, 1.0), name
    assert float(ent.abs().max()) > 0


def test_the_recurrent_agent_steps_and_windows_like_the_start_kits(run):
    _, obs, _, _, _, _ = run
    torch.manual_seed(3)
    r = RecurrentReducedAgent(T, H, input_size=I, query_scale=0.125).double()
    with torch.no_grad():
        a, lp, ent, v, state = r(obs)
        assert tuple(a.shape) == (N, 12) and tuple(state[0].shape) == (1, N, H)
        window = torch.stack([obs, obs], 1)
        a2 = torch.stack([a, a], 1)
        _, lp2, _, v2, _ = r(window, action=a2)
        assert tuple(lp2.shape) == (2 * N,) and torch.allclose(lp2.view(N, 2)[:, 0], r(obs, action=a)[1])
    r.seed, r.query_scale = 7, 0.5
    assert (r.policy.seed, r.policy.query_scale) == (7, 0.5)


@pytest.mark.parametrize("flags", [dict(fused_heads=True), dict(fused_tile=True),
                                   dict(fused_tile=True, fused_tile_conv2=True), dict(fused_item=True),
                                   dict(fused_player=True)])
def test_every_fused_flag_on_host_tensors_is_an_error(flags):
    agent = ReducedAgent(T, I, H, **flags)
    obs, _ = make_rows(5, seed=1, task_dim=T)
    with pytest.raises(HeadsError):
        with torch.no_grad():
            agent(obs)
    with pytest.raises(TypeError):
        ReducedAgent(T, I, H, fused_decoder=True)  # there is no one-launch decoder for this policy
