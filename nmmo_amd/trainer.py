"""Device-resident evaluate/train loop around the HIP stepper and the HBM experience storage.

The reference trainer (`reinforcement_learning/clean_pufferl.py`) runs `evaluate(data)` — recv,
policy forward, copy the learner-mask rows into host storage, send (`:287-357`) — and then
`train(data)` — sort the (env_id, step) keys, the reversed GAE loop, flatten the batch and run
`update_epochs` of PPO minibatches (`:390-540`). `DeviceTrainer` keeps that control flow and
those names, but nothing leaves the GPU: recv is the engine's obs/reward/done/mask tensors in
HBM (`NmmoEngine`, the HIP tick + obs kernels), the stores, sort, advantages and minibatch
gathers are the `nmmo_exp_*` kernels (`DeviceExperience`, `csrc/storage.hip`), and send is
`nmmo_step` on the sampled actions. The PPO loss and optimizer step are the reference's
expressions (`:476-523`) on whatever agent the caller passes.

The policy networks themselves are out of scope (consumers of the path);
`MaskedLinearAgent` is a minimal stand-in with the reference policies' call convention —
`agent(obs, action=None) -> (action, logprob, entropy, value)` with every head's logits masked
by the obs ActionTargets (baseline_policy.py:245-262) — so the loop can be exercised and timed.
`PointerMaskedAgent` is the same stand-in with the reference decoders' pointer heads
(baseline_policy.py:222-230; SPEC.md §18).
`TileMaskedAgent` is the same stand-in behind the reference's tile encoder
(baseline_policy.py:85-112; SPEC.md §19).
`ItemMaskedAgent` is the same stand-in with the reference's item path: the item encoder over
Inventory and Market, their pooled embeddings and the five item pointer heads
(baseline_policy.py:47-51, 148-190; SPEC.md §20).
`PlayerMaskedAgent` is the same stand-in with the reference's player path: the player encoder over
Entity, its pooled embedding, the row's own entity and the three entity pointer heads
(baseline_policy.py:43-45, 115-145; SPEC.md §21).
`RecurrentMaskedAgent` is the same stand-in with an LSTM between encoder and heads and the
reference's recurrent convention, `agent(obs, state, action=None) -> (..., state)`: for an agent
with an `.lstm` attribute the loop carries one LSTM state per agent slot through `evaluate()` and
trains over `[batch_rows, bptt_horizon]` windows, the state handed from one minibatch to the next
(clean_pufferl.py:177-182, :310-324, :454-469; SPEC.md §17).
"""

from __future__ import annotations

import dataclasses
import math
import time

import numpy as np
import torch
from torch import nn

from . import layout
from .storage import DeviceExperience


@dataclasses.dataclass
class TrainConfig:
    """The `train:` section of the reference's config.yaml (names and defaults)."""

    seed: int = 1
    total_timesteps: int = 10_000_000
    learning_rate: float = 1.5e-4
    anneal_lr: bool = True
    gamma: float = 0.99
    gae_lambda: float = 0.95
    update_epochs: int = 3
    norm_adv: bool = True
    clip_coef: float = 0.1
    clip_vloss: bool = True
    ent_coef: float = 0.01
    vf_coef: float = 0.5
    max_grad_norm: float = 0.5
    target_kl: float | None = None
    batch_size: int = 32768
    batch_rows: int = 128
    bptt_horizon: int = 8
    vf_clip_coef: float = 0.1
    # the minibatch loss as one `ppo.ppo_loss` call (the HIP kernel of SPEC.md §16) instead of the
    # chain of torch ops; not part of the reference's config
    fused_loss: bool = False

    def validate(self):
        if self.batch_size % (self.bptt_horizon * self.batch_rows):
            raise ValueError("batch_size must be a multiple of bptt_horizon * batch_rows (clean_pufferl.py:412)")


class MaskedLinearAgent(nn.Module):
    """A small stand-in policy: the 15x15 Tile materials and the agent's own tick through one
    hidden layer, a linear head per action with illegal entries masked out by the obs's
    ActionTargets, and a value head.

    `fused_heads=True` runs the heads as one `heads.masked_heads` call (the HIP kernels of
    SPEC.md §15) instead of the loop of Categoricals; sampling then draws from philox under
    `seed` with a counter that advances on every sampling call, not from torch's generator, and
    sampled actions are int32."""

    def __init__(self, task_dim: int = 2048, hidden: int = 64, fused_heads: bool = False, seed: int = 0):
        super().__init__()
        self.fused_heads = bool(fused_heads)
        self.seed = int(seed)
        self.draws = 0  # sampling calls so far: the `offset` of the next one
        lay = layout.flat_layout(task_dim)
        self.o_tile = lay["Tile"].offset
        self.o_tick = lay["CurrentTick"].offset
        self.dims = list(layout.ACTION_DIMS)
        self.mask_off = np.cumsum([0] + self.dims).tolist()
        self.encoder = nn.Sequential(nn.Linear(layout.TILE_ROWS + 1, hidden), nn.ReLU())
        self.actor = nn.Linear(hidden, sum(self.dims))
        self.value = nn.Linear(hidden, 1)

    def forward(self, obs: torch.Tensor, action: torch.Tensor | None = None):
        mat = obs[:, self.o_tile + 2:self.o_tile + 3 * layout.TILE_ROWS:3] / 16.0
        tick = obs[:, self.o_tick:self.o_tick + 1] / 1024.0
        return self.heads(self.encoder(torch.cat([mat, tick], 1)), obs, action)

    def heads(self, h: torch.Tensor, obs: torch.Tensor, action: torch.Tensor | None = None):
        """The masked action heads and the value head on the hidden rows `h` of the rows `obs`."""
        return self.masked(self.actor(h), h, obs, action)

    def masked(self, logits: torch.Tensor, h: torch.Tensor, obs: torch.Tensor, action: torch.Tensor | None = None):
        """`heads` from the heads' concatenated logits on."""
        if self.fused_heads:
            from .heads import masked_heads

            acts, logp, ent = masked_heads(logits, obs, self.dims, action, seed=self.seed, offset=self.draws)
            if action is None:
                self.draws += 1
            return acts, logp, ent, self.value(h)
        masks = obs[:, :self.mask_off[-1]] > 0
        acts, logp, ent = [], 0.0, 0.0
        for k, n in enumerate(self.dims):
            lo, hi = self.mask_off[k], self.mask_off[k + 1]
            lg = logits[:, lo:hi].masked_fill(~masks[:, lo:hi], -1e9)
            dist = torch.distributions.Categorical(logits=lg)
            a = dist.sample() if action is None else action[:, k]
            acts.append(a)
            logp = logp + dist.log_prob(a)
            ent = ent + dist.entropy()
        return torch.stack(acts, 1), logp, ent, self.value(h)


def pointer_logits(queries, keys, head_set, dense, dims):
    """The heads' logits [N, sum(dims)] materialised the reference's way (baseline_policy.py:58-70,
    :222-230): a zero embedding for the no-op appended to every key set, one batched mat-vec per
    pointer head, the dense heads' logits in between. Arguments as for `heads.pointer_heads`."""
    padded = [torch.cat([k, k.new_zeros(k.shape[0], 1, k.shape[2])], 1) for k in keys]
    parts, p, d = [], 0, 0
    for size, s in zip(dims, head_set):
        if s < 0:
            parts.append(dense[:, d:d + size])
            d += size
        else:
            parts.append(torch.matmul(padded[s], queries[:, p].unsqueeze(-1)).squeeze(-1))
            p += 1
    return torch.cat(parts, 1)


class PointerMaskedAgent(MaskedLinearAgent):
    """The stand-in with the decoder shape of the reference's policies (baseline_policy.py:58-70,
    :222-230; SPEC.md §18): the eight heads that choose an entity, an inventory slot or a market
    listing are pointer heads. Each takes its logits as the dot products of a query, a
    `Linear(hidden, hidden)` of the hidden row, with the row's candidate embeddings, a
    `Linear(cols, hidden)` over the row's Entity [100, 31], Inventory [12, 16] or Market [1024, 16]
    section (squashed by tanh(x / 64), the query scaled by 1 / sqrt(hidden): the logits stay within
    a few units), plus a zero logit for the no-op entry. The four other heads keep a `Linear(hidden, n)`.

    `fused_pointer=True` runs all twelve heads as one `heads.pointer_heads` call (philox draws,
    `draws` and int32 actions as with `fused_heads`); otherwise the logits are materialised the
    reference's way, `cat` of a zero row and `matmul`, and go through the parent's path.

    The market keys alone are 256 KB per row at hidden 64: this stand-in is for the loop's small
    shapes, not for the 131,072 rows of C4."""

    SETS = (("Entity", ("Attack.Target", "Give.Target", "GiveGold.Target")),
            ("Inventory", ("Destroy.InventoryItem", "Give.InventoryItem", "Sell.InventoryItem", "Use.InventoryItem")),
            ("Market", ("Buy.MarketItem",)))

    def __init__(self, task_dim: int = 2048, hidden: int = 64, fused_heads: bool = False, seed: int = 0,
                 fused_pointer: bool = False):
        super().__init__(task_dim, hidden, fused_heads, seed)
        del self.actor  # every head has its own layer below
        self.fused_pointer = bool(fused_pointer)
        lay = layout.flat_layout(task_dim)
        self.sections = [(lay[name].offset, *lay[name].shape) for name, _ in self.SETS]
        self.head_set = [-1] * len(self.dims)
        for s, (_, names) in enumerate(self.SETS):
            for name in names:
                self.head_set[layout.HEAD[name]] = s
        self.key_encoders = nn.ModuleList(nn.Linear(cols, hidden) for _, _, cols in self.sections)
        self.queries = nn.ModuleList(nn.Linear(hidden, hidden) for s in self.head_set if s >= 0)
        self.dense = nn.ModuleList(nn.Linear(hidden, n) for n, s in zip(self.dims, self.head_set) if s < 0)
        self.query_scale = 1.0 / math.sqrt(hidden)

    def heads(self, h: torch.Tensor, obs: torch.Tensor, action: torch.Tensor | None = None):
        n = obs.shape[0]
        keys = [enc(torch.tanh(obs[:, o:o + rows * cols].reshape(n, rows, cols) / 64.0))
                for enc, (o, rows, cols) in zip(self.key_encoders, self.sections)]
        queries = torch.stack([q(h) for q in self.queries], 1) * self.query_scale
        dense = torch.cat([d(h) for d in self.dense], 1)
        if self.fused_pointer:
            from .heads import pointer_heads

            acts, logp, ent = pointer_heads(queries, keys, self.head_set, dense, obs, self.dims, action,
                                            seed=self.seed, offset=self.draws)
            if action is None:
                self.draws += 1
            return acts, logp, ent, self.value(h)
        return self.masked(pointer_logits(queries, keys, self.head_set, dense, self.dims), h, obs, action)


class TileMaskedAgent(MaskedLinearAgent):
    """The stand-in with the observation encoder every reference policy starts with: the
    reference's `TileEncoder` (baseline_policy.py:85-112: 225 x 3 embeddings, two convolutions, a
    linear layer; `nmmo_amd/tile.py`) over the row's Tile section, then the tick and one hidden
    layer as in the parent. `fused_tile=True` runs the embedding, the first convolution and its
    ReLU as one `tile.tile_conv1` call (the HIP kernels of SPEC.md §19), reading the obs rows in
    place; `fused_tile_conv2=True` (with `fused_tile`) runs the second convolution and its ReLU in
    that kernel too (`tile.tile_conv12`, SPEC.md §22). The call convention is the parent's."""

    def __init__(self, task_dim: int = 2048, hidden: int = 64, fused_heads: bool = False, seed: int = 0,
                 fused_tile: bool = False, fused_tile_conv2: bool = False):
        super().__init__(task_dim, hidden, fused_heads, seed)
        from .tile import TileEncoder

        self.tile_encoder = TileEncoder(hidden, fused=fused_tile, fused_conv2=fused_tile_conv2)
        self.encoder = nn.Sequential(nn.Linear(hidden + 1, hidden), nn.ReLU())

    def forward(self, obs: torch.Tensor, action: torch.Tensor | None = None):
        tick = obs[:, self.o_tick:self.o_tick + 1] / 1024.0
        return self.heads(self.encoder(torch.cat([self.tile_encoder(obs, self.o_tile), tick], 1)), obs, action)


class ItemMaskedAgent(MaskedLinearAgent):
    """The stand-in with the reference's item path (baseline_policy.py:47-51, 148-190, 222-230;
    `nmmo_amd/item.py`, SPEC.md §20): one `ItemEncoder` over the row's Inventory [12, 16] and Market
    [1024, 16] sections. The hidden row is the parent's (materials and tick) plus a
    `Linear(12 hidden, hidden)` over the inventory embeddings (`InventoryEncoder`) plus a
    `Linear(hidden, hidden)` over the pooled market embedding (`MarketEncoder`). The four
    `*.InventoryItem` heads and `Buy.MarketItem` are pointer heads over the item embeddings, each
    with a `Linear(hidden, hidden)` query scaled by 1 / sqrt(hidden) as in `PointerMaskedAgent`;
    the other seven heads keep a `Linear(hidden, n)`. Either way the [N, 1586] logits go through the
    parent's `masked`, so `fused_heads` works with both.

    `fused_item=False` materialises the embeddings, pads the zero row and uses `matmul`, the
    reference's way: 256 KB of market embeddings per row at hidden 64. `fused_item=True` makes one
    `item.item_logits` call per set and one `item.item_sums` call, reading the obs rows in place,
    and holds no [N, 1024, .] tensor. The call convention is the parent's."""

    SETS = (("Inventory", ("Destroy.InventoryItem", "Give.InventoryItem", "Sell.InventoryItem", "Use.InventoryItem")),
            ("Market", ("Buy.MarketItem",)))

    def __init__(self, task_dim: int = 2048, hidden: int = 64, fused_heads: bool = False, seed: int = 0,
                 fused_item: bool = False):
        super().__init__(task_dim, hidden, fused_heads, seed)
        from .item import ItemEncoder

        del self.actor  # every head has its own layer below
        lay = layout.flat_layout(task_dim)
        self.sections = [(lay[name].offset, *lay[name].shape) for name, _ in self.SETS]
        self.set_heads = [[layout.HEAD[name] for name in names] for _, names in self.SETS]
        pointer = sorted(k for ks in self.set_heads for k in ks)
        self.query_of = {k: p for p, k in enumerate(pointer)}  # head -> its row of `queries`
        self.item_encoder = ItemEncoder(hidden, fused=fused_item)
        self.inventory = nn.Linear(layout.INVENTORY_N_OBS * hidden, hidden)
        self.market = nn.Linear(hidden, hidden)
        self.queries = nn.ModuleList(nn.Linear(hidden, hidden) for _ in pointer)
        self.dense = nn.ModuleList(nn.Linear(hidden, n) for k, n in enumerate(self.dims) if k not in self.query_of)
        self.query_scale = 1.0 / math.sqrt(hidden)

    def item_sets(self, obs: torch.Tensor):
        """The rows' Inventory and Market sections, as views of `obs`."""
        return [obs[:, o:o + rows * cols] for o, rows, cols in self.sections]

    def hidden(self, obs: torch.Tensor):
        """(the hidden rows, the inventory embeddings [N, 12, H], the market embeddings [N, 1024, H]
        or None on the fused path)."""
        mat = obs[:, self.o_tile + 2:self.o_tile + 3 * layout.TILE_ROWS:3] / 16.0
        tick = obs[:, self.o_tick:self.o_tick + 1] / 1024.0
        inv, mk = self.item_sets(obs)
        enc = self.item_encoder
        inv_emb = enc.embed(inv)
        if enc.fused:
            mk_emb, market = None, self.market(enc.pooled(mk))
        else:
            mk_emb = enc.embed(mk)
            market = self.market(mk_emb).mean(-2)
        return self.encoder(torch.cat([mat, tick], 1)) + self.inventory(inv_emb.flatten(1)) + market, inv_emb, mk_emb

    def forward(self, obs: torch.Tensor, action: torch.Tensor | None = None):
        h, inv_emb, mk_emb = self.hidden(obs)
        return self.masked(self.logits(h, obs, inv_emb, mk_emb), h, obs, action)

    def heads(self, h: torch.Tensor, obs: torch.Tensor, action: torch.Tensor | None = None):
        inv, mk = self.item_sets(obs)
        enc = self.item_encoder
        embs = (None, None) if enc.fused else (enc.embed(inv), enc.embed(mk))
        return self.masked(self.logits(h, obs, *embs), h, obs, action)

    def logits(self, h, obs, inv_emb=None, mk_emb=None):
        """The twelve heads' logits [N, 1586] in head order. The unfused path takes the item
        embeddings; the fused path reads the rows (its illegal and no-op entries are 0)."""
        queries = torch.stack([q(h) for q in self.queries], 1) * self.query_scale  # [N, 5, H]
        parts = [None] * len(self.dims)
        dense = iter(self.dense)
        for k in range(len(self.dims)):
            if k not in self.query_of:
                parts[k] = next(dense)(h)
        if self.item_encoder.fused:
            from .item import item_logits

            pq = self.item_encoder.pointer_query(queries)
            for items, ks in zip(self.item_sets(obs), self.set_heads):
                rows = self.dims[ks[0]]
                lg = item_logits(items, pq[:, [self.query_of[k] for k in ks]], obs, [self.mask_off[k] for k in ks])
                for i, k in enumerate(ks):
                    parts[k] = lg[:, i * rows:(i + 1) * rows]
        else:
            for emb, ks in zip((inv_emb, mk_emb), self.set_heads):
                padded = torch.cat([emb, emb.new_zeros(emb.shape[0], 1, emb.shape[2])], 1)
                for k in ks:
                    parts[k] = torch.matmul(padded, queries[:, self.query_of[k]].unsqueeze(-1)).squeeze(-1)
        return torch.cat(parts, 1)


class PlayerMaskedAgent(MaskedLinearAgent):
    """The stand-in with the reference's player path (baseline_policy.py:43-45, 52, 115-145, 222-230;
    `nmmo_amd/player.py`, SPEC.md §21): a `PlayerEncoder` over the row's Entity [100, 31] section and
    its AgentId. The hidden row is the parent's (materials and tick) plus a `Linear(hidden, hidden)`
    over the pooled entity embedding plus a `Linear(hidden, hidden)` over `my_agent`, the embedding of
    the row's own entity. The three `*.Target` heads are pointer heads over the entity embeddings,
    each with a `Linear(hidden, hidden)` query scaled by 1 / sqrt(hidden) as in `PointerMaskedAgent`;
    the other nine heads keep a `Linear(hidden, n)`. Either way the [N, 1586] logits go through the
    parent's `masked`, so `fused_heads` works with both.

    `fused_player=False` materialises the embeddings, pads the zero row and uses `matmul`, the
    reference's way: 25 KB of entity embeddings per row at hidden 64. `fused_player=True` makes one
    `player.player_own`, one `player.player_sums` and one `player.player_logits` call, reading the obs
    rows in place, and holds no [N, 100, .] tensor. The call convention is the parent's."""

    TARGETS = ("Attack.Target", "Give.Target", "GiveGold.Target")

    def __init__(self, task_dim: int = 2048, hidden: int = 64, fused_heads: bool = False, seed: int = 0,
                 fused_player: bool = False):
        super().__init__(task_dim, hidden, fused_heads, seed)
        from .player import PlayerEncoder

        del self.actor  # every head has its own layer below
        lay = layout.flat_layout(task_dim)
        self.o_entity, self.o_id = lay["Entity"].offset, lay["AgentId"].offset
        self.target_heads = [layout.HEAD[name] for name in self.TARGETS]
        self.query_of = {k: p for p, k in enumerate(sorted(self.target_heads))}  # head -> its row of `queries`
        self.player_encoder = PlayerEncoder(hidden, hidden, fused=fused_player)
        self.players = nn.Linear(hidden, hidden)
        self.my_agent = nn.Linear(hidden, hidden)
        self.queries = nn.ModuleList(nn.Linear(hidden, hidden) for _ in self.target_heads)
        self.dense = nn.ModuleList(nn.Linear(hidden, n) for k, n in enumerate(self.dims) if k not in self.query_of)
        self.query_scale = 1.0 / math.sqrt(hidden)

    def entities(self, obs: torch.Tensor):
        """The rows' Entity sections and AgentId elements, as views of `obs`."""
        return obs[:, self.o_entity:self.o_entity + layout.PLAYER_N_OBS * layout.ENTITY_COLS], obs[:, self.o_id]

    def hidden(self, obs: torch.Tensor):
        """(the hidden rows, the entity embeddings [N, 100, H] or None on the fused path)."""
        mat = obs[:, self.o_tile + 2:self.o_tile + 3 * layout.TILE_ROWS:3] / 16.0
        tick = obs[:, self.o_tick:self.o_tick + 1] / 1024.0
        ents, ids = self.entities(obs)
        enc = self.player_encoder
        if enc.fused:
            emb, pooled = None, enc.pooled(ents)
        else:
            emb = enc.embed(ents)
            pooled = emb.mean(1)
        h = self.encoder(torch.cat([mat, tick], 1)) + self.players(pooled) + self.my_agent(enc.my_agent(ents, ids))
        return h, emb

    def forward(self, obs: torch.Tensor, action: torch.Tensor | None = None):
        h, emb = self.hidden(obs)
        return self.masked(self.logits(h, obs, emb), h, obs, action)

    def heads(self, h: torch.Tensor, obs: torch.Tensor, action: torch.Tensor | None = None):
        enc = self.player_encoder
        emb = None if enc.fused else enc.embed(self.entities(obs)[0])
        return self.masked(self.logits(h, obs, emb), h, obs, action)

    def logits(self, h, obs, emb=None):
        """The twelve heads' logits [N, 1586] in head order. The unfused path takes the entity
        embeddings; the fused path reads the rows (its illegal and no-op entries are 0)."""
        queries = torch.stack([q(h) for q in self.queries], 1) * self.query_scale  # [N, 3, H]
        parts = [None] * len(self.dims)
        dense = iter(self.dense)
        for k in range(len(self.dims)):
            if k not in self.query_of:
                parts[k] = next(dense)(h)
        ks = sorted(self.target_heads)
        if self.player_encoder.fused:
            from .player import player_logits

            width = layout.PLAYER_N_OBS + 1
            pq = self.player_encoder.pointer_query(queries)
            lg = player_logits(self.entities(obs)[0], pq, obs, [self.mask_off[k] for k in ks])
            for k in ks:
                parts[k] = lg[:, self.query_of[k] * width:(self.query_of[k] + 1) * width]
        else:
            padded = torch.cat([emb, emb.new_zeros(emb.shape[0], 1, emb.shape[2])], 1)
            for k in ks:
                parts[k] = torch.matmul(padded, queries[:, self.query_of[k]].unsqueeze(-1)).squeeze(-1)
        return torch.cat(parts, 1)


class RecurrentMaskedAgent(MaskedLinearAgent):
    """The stand-in with an LSTM between its encoder and its heads, in the calling convention of
    the reference's recurrent policies (pufferlib's Recurrent wrapper; clean_pufferl.py:317-324,
    :465-469): `agent(obs, state=None, action=None) -> (action, logprob, entropy, value, state)`.

    obs is [B, E] (one step) or [B, T, E] (a window); the four outputs are flattened in (B, T)
    order; state is (h, c), each [num_layers, B, hidden]. `fused_lstm=True` runs the recurrence
    as `lstm.LSTM` (the HIP kernels of SPEC.md §17) instead of `torch.nn.LSTM`: under
    `torch.no_grad()` a given state is then updated in place and returned."""

    def __init__(self, task_dim: int = 2048, hidden: int = 64, fused_heads: bool = False, seed: int = 0,
                 fused_lstm: bool = False, num_layers: int = 1):
        super().__init__(task_dim, hidden, fused_heads, seed)
        self.fused_lstm = bool(fused_lstm)
        if self.fused_lstm:
            from .lstm import LSTM

            self.lstm = LSTM(hidden, hidden, num_layers)
        else:
            self.lstm = nn.LSTM(hidden, hidden, num_layers)

    def hidden(self, obs: torch.Tensor, state=None):
        """Encoder and LSTM: (hidden rows [B * T, hidden] in (B, T) order, the obs rows in that
        order, the new state)."""
        B, T = obs.shape[0], (obs.shape[1] if obs.dim() == 3 else 1)
        flat = obs.reshape(B * T, obs.shape[-1])
        mat = flat[:, self.o_tile + 2:self.o_tile + 3 * layout.TILE_ROWS:3] / 16.0
        tick = flat[:, self.o_tick:self.o_tick + 1] / 1024.0
        x = self.encoder(torch.cat([mat, tick], 1)).view(B, T, -1).transpose(0, 1)  # time first
        if self.fused_lstm and state is not None and not torch.is_grad_enabled():
            y, state = self.lstm(x, state, out=state)
        else:
            y, state = self.lstm(x, state)
        return y.transpose(0, 1).reshape(B * T, -1), flat, state

    def forward(self, obs: torch.Tensor, state=None, action: torch.Tensor | None = None):
        h, flat, state = self.hidden(obs, state)
        if action is not None:
            action = action.reshape(h.shape[0], -1)
        return (*self.heads(h, flat, action), state)


class DeviceTrainer:
    """clean_pufferl's evaluate()/train() over one NmmoEngine (flat obs) and DeviceExperience."""

    def __init__(self, engine, agent: nn.Module, config: TrainConfig, env_id_base: int = 0):
        config.validate()
        self.engine = engine
        self.agent = agent
        self.config = config
        self.device = engine.device
        self.n_rows = engine.n_envs * engine.P
        self.env_id_base = int(env_id_base)
        self.experience = DeviceExperience(config.batch_size, engine.obs_elems, self.n_rows, device=self.device)
        self.optimizer = torch.optim.Adam(agent.parameters(), lr=config.learning_rate, eps=1e-5)
        self.total_updates = max(1, config.total_timesteps // config.batch_size)
        self.update = 0
        self.global_step = 0
        self.agent_step = 0
        self.last_batch = None
        self.stats = {}
        # one LSTM state per agent slot (clean_pufferl.py:177-182), carried across evaluate() calls
        # and, as in the reference, not reset when an agent dies or an env resets
        self.next_lstm_state = None
        if hasattr(agent, "lstm"):
            shape = (agent.lstm.num_layers, self.n_rows, agent.lstm.hidden_size)
            self.next_lstm_state = (torch.zeros(shape, device=self.device), torch.zeros(shape, device=self.device))

    def evaluate(self, on_store=None) -> dict:
        """One batch of experience (clean_pufferl.py:287-357): recv -> forward -> store -> send
        until ptr == batch_size + 1. Returns the reference's SPS counters. `on_store(o, r, d,
        mask, actions, logprob, value, env_id, step)` (optional, for checkers) sees each store's
        inputs before the step overwrites them."""
        eng, exp = self.engine, self.experience
        exp.reset()
        N = self.n_rows
        agent_steps = torch.zeros((), dtype=torch.int64, device=self.device)
        padded = step = 0
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        while not exp.full():
            step += 1
            o = eng.obs.view(N, eng.obs_elems)
            r, d, mask = eng.rew.view(N), eng.term.view(N), eng.mask.view(N)
            with torch.no_grad():
                if self.next_lstm_state is not None:
                    # rows are in identity order: no gather or scatter by env_id (:310-324)
                    actions, logprob, _, value, self.next_lstm_state = self.agent(o, self.next_lstm_state)
                else:
                    actions, logprob, _, value = self.agent(o)
            agent_steps += mask.sum()
            padded += N
            exp.store(o, r, d, mask, actions, logprob, value.flatten(), step, env_id_base=self.env_id_base)
            if on_store is not None:
                on_store(o, r, d, mask, actions, logprob, value.flatten(),
                         self.env_id_base + torch.arange(N, device=self.device), step)
            eng.step(actions.to(torch.int32).view(eng.n_envs, eng.P, -1))
        torch.cuda.synchronize(self.device)
        elapsed = time.perf_counter() - t0
        eng.check_fault("DeviceTrainer.evaluate")  # the batch boundary: no faulted tick reaches train()
        agent_steps = int(agent_steps.item())
        self.agent_step += agent_steps
        self.global_step += padded
        self.stats = {"SPS": int(padded / elapsed), "agent_SPS": int(agent_steps / elapsed),
                      "agent_steps": agent_steps, "padded_steps": padded, "eval_time": elapsed,
                      "reward": float(exp.rewards[:exp.batch_size].mean())}
        return self.stats

    def train(self) -> dict:
        """One update (clean_pufferl.py:390-540): sort, GAE, flatten, PPO epochs."""
        cfg, exp, agent = self.config, self.experience, self.agent
        if cfg.anneal_lr:
            # clean_pufferl.py:409 with data.update counted from 0 and incremented after train()
            # (:140, :557): the first update's frac is 1 + 1/total_updates, as in the reference
            frac = 1.0 - (self.update - 1.0) / self.total_updates
            self.optimizer.param_groups[0]["lr"] = frac * cfg.learning_rate
        t0 = time.perf_counter()
        idxs = exp.sort()
        advantages = exp.advantages(idxs, cfg.gamma, cfg.gae_lambda)
        b = exp.batch(idxs, advantages, cfg.batch_rows, cfg.bptt_horizon)
        self.last_batch = (idxs, advantages, b)
        b_returns, b_values, b_adv = b["b_returns"], b["b_values"], b["b_advantages"]
        pg_losses, entropy_losses, v_losses, clipfracs, old_kls, kls = [], [], [], [], [], []
        approx_kl = None
        if cfg.fused_loss:
            from . import ppo

            acc = ppo.new_accumulator(self.device)  # the minibatch stats are summed on the device
        recurrent = hasattr(agent, "lstm")
        for _ in range(cfg.update_epochs):
            lstm_state = None  # clean_pufferl.py:455
            for mb in range(b["num_minibatches"]):
                m = exp.minibatch(b["b_idxs"], mb)
                mb_actions = m["actions"].reshape(-1, m["actions"].shape[-1])
                mb_values = b_values[mb].reshape(-1)
                mb_advantages = b_adv[mb].reshape(-1)
                mb_returns = b_returns[mb].reshape(-1)
                if recurrent:
                    # [batch_rows, bptt_horizon, obs_elems]; the state goes on to the next minibatch (:465-469)
                    mb_obs = m["obs"].reshape(cfg.batch_rows, cfg.bptt_horizon, exp.obs_elems)
                    _, newlogprob, entropy, newvalue, lstm_state = agent(mb_obs, state=lstm_state, action=mb_actions)
                    lstm_state = (lstm_state[0].detach(), lstm_state[1].detach())
                else:
                    mb_obs = m["obs"].reshape(-1, exp.obs_elems)
                    _, newlogprob, entropy, newvalue = agent(mb_obs, action=mb_actions)
                if cfg.fused_loss:
                    loss, st = ppo.ppo_loss(
                        newlogprob, entropy, newvalue.view(-1), m["logprobs"].reshape(-1), mb_advantages, mb_returns,
                        mb_values, clip_coef=cfg.clip_coef, vf_clip_coef=cfg.vf_clip_coef, ent_coef=cfg.ent_coef,
                        vf_coef=cfg.vf_coef, norm_adv=cfg.norm_adv, clip_vloss=cfg.clip_vloss, accum=acc)
                    approx_kl = st[ppo.APPROX_KL]
                    self.optimizer.zero_grad()
                    loss.backward()
                    nn.utils.clip_grad_norm_(agent.parameters(), cfg.max_grad_norm)
                    self.optimizer.step()
                    continue
                logratio = newlogprob - m["logprobs"].reshape(-1)
                ratio = logratio.exp()
                with torch.no_grad():
                    old_kls.append((-logratio).mean())
                    approx_kl = ((ratio - 1) - logratio).mean()
                    kls.append(approx_kl)
                    clipfracs.append(((ratio - 1.0).abs() > cfg.clip_coef).float().mean())
                if cfg.norm_adv:
                    mb_advantages = (mb_advantages - mb_advantages.mean()) / (mb_advantages.std() + 1e-8)
                pg_loss1 = -mb_advantages * ratio
                pg_loss2 = -mb_advantages * torch.clamp(ratio, 1 - cfg.clip_coef, 1 + cfg.clip_coef)
                pg_loss = torch.max(pg_loss1, pg_loss2).mean()
                newvalue = newvalue.view(-1)
                if cfg.clip_vloss:
                    v_loss_unclipped = (newvalue - mb_returns) ** 2
                    v_clipped = mb_values + torch.clamp(newvalue - mb_values, -cfg.vf_clip_coef, cfg.vf_clip_coef)
                    v_loss_clipped = (v_clipped - mb_returns) ** 2
                    v_loss = 0.5 * torch.max(v_loss_unclipped, v_loss_clipped).mean()
                else:
                    v_loss = 0.5 * ((newvalue - mb_returns) ** 2).mean()
                entropy_loss = entropy.mean()
                loss = pg_loss - cfg.ent_coef * entropy_loss + v_loss * cfg.vf_coef
                self.optimizer.zero_grad()
                loss.backward()
                nn.utils.clip_grad_norm_(agent.parameters(), cfg.max_grad_norm)
                self.optimizer.step()
                pg_losses.append(pg_loss.detach())
                v_losses.append(v_loss.detach())
                entropy_losses.append(entropy_loss.detach())
            if cfg.target_kl is not None and approx_kl is not None and approx_kl > cfg.target_kl:
                break
        y_pred, y_true = b_values.reshape(-1), b_returns.reshape(-1)
        var_y = torch.var(y_true, unbiased=False)
        explained_var = float("nan") if float(var_y) == 0 else float(1 - torch.var(y_true - y_pred, unbiased=False) / var_y)
        mean = lambda xs: float(torch.stack(xs).mean()) if xs else math.nan  # noqa: E731
        losses = {"policy_loss": mean(pg_losses), "value_loss": mean(v_losses), "entropy": mean(entropy_losses),
                  "old_approx_kl": mean(old_kls), "approx_kl": mean(kls), "clipfrac": mean(clipfracs),
                  "explained_variance": explained_var}
        if cfg.fused_loss:  # one host read for all of them
            sums = acc.tolist()
            for key, k in (("policy_loss", ppo.PG_LOSS), ("value_loss", ppo.V_LOSS), ("entropy", ppo.ENTROPY),
                           ("old_approx_kl", ppo.OLD_APPROX_KL), ("approx_kl", ppo.APPROX_KL),
                           ("clipfrac", ppo.CLIPFRAC)):
                losses[key] = sums[k] / sums[ppo.N_STATS] if sums[ppo.N_STATS] else math.nan
        torch.cuda.synchronize(self.device)
        self.update += 1
        losses["train_time"] = time.perf_counter() - t0
        losses["train_sps"] = int(cfg.batch_size / losses["train_time"])
        return losses
