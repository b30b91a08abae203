"""The start-kit `Baseline` policy (baseline_policy.py:22-82) assembled from this package's modules:
six encoders into `proj_fc`, the twelve decoder layers and a value head, with the reference's
parameter names and shapes, so that a start-kit policy `state_dict` loads with `strict=True`.

    agent = BaselineAgent(task_dim, hidden=256, fused_decoder=True, ...).cuda()
    action, logprob, entropy, value = agent(obs)                 # sample
    _, logprob, entropy, value = agent(obs, action=action)       # evaluate
    action, logprob, entropy, value = agent(obs, greedy=True)    # select: every head's first maximum

`RecurrentBaselineAgent` is the policy the start kit trains, `Recurrent(Baseline)`: this one as `policy`
and an LSTM as `recurrent`, in the recurrent calling convention.

The call convention is the stand-ins' of `nmmo_amd/trainer.py`, which `DeviceTrainer` takes: `obs` is
the flat obs rows [N, obs_elems] float32, read through views and never written (the reference's tile
encoder edits its argument in place; `tile.TileEncoder` does not).

Every `fused_*` flag swaps one part for its HIP path and none changes a parameter:
`fused_tile` / `fused_tile_conv2` (SPEC.md §19, §22), `fused_item` (§20: pooled item features, and
`item_logits` where the decoder is not fused), `fused_player` (§21: own row, pooled entity features,
and `player_logits` likewise), `fused_heads` (§15) and `fused_decoder` (§23: all twelve heads from the
obs rows in one `decoder.decoder_heads` call; it needs none of the others). With `fused_heads` or
`fused_decoder` sampling draws from philox under `seed` with the counter `draws`, which advances on
every sampling call, and sampled actions are int32.

As in the reference, `inventory_encoder.fc` exists (a start-kit `state_dict` has it) and the forward
does not use it: the inventory enters `proj_fc` as the mean of its item embeddings.
"""

from __future__ import annotations

import numpy as np
import torch
from torch import nn

from . import layout
from .item import ItemEncoder
from .player import PlayerEncoder
from .tile import TileEncoder

# the reference's ActionDecoder.layers in its order, which is the order of layout.ACTION_HEADS:
# (name, the candidate set a pointer head points into or None for a dense head)
DECODER_LAYERS = (("attack_style", None), ("attack_target", "Entity"), ("market_buy", "Market"),
                  ("inventory_destroy", "Inventory"), ("inventory_give_item", "Inventory"),
                  ("inventory_give_player", "Entity"), ("gold_quantity", None), ("gold_target", "Entity"),
                  ("move", None), ("inventory_sell", "Inventory"), ("inventory_price", None),
                  ("inventory_use", "Inventory"))
SETS = ("Entity", "Inventory", "Market")  # the decoder call's candidate sets, in this order


class _Fc(nn.Module):
    """A reference encoder that is one linear layer named `fc`."""

    def __init__(self, n_in: int, n_out: int):
        super().__init__()
        self.fc = nn.Linear(n_in, n_out)


class ActionDecoder(nn.Module):
    """The reference's twelve layers (baseline_policy.py:202-220): `Linear(hidden, n)` for a dense head,
    `Linear(hidden, hidden)`, the query, for a pointer head."""

    def __init__(self, hidden: int, dims):
        super().__init__()
        self.layers = nn.ModuleDict({name: nn.Linear(hidden, hidden if s is not None else n)
                                     for (name, s), n in zip(DECODER_LAYERS, dims)})


class BaselineAgent(nn.Module):
    def __init__(self, task_dim: int = 2048, hidden: int = 256, *, fused_heads: bool = False,
                 fused_tile: bool = False, fused_tile_conv2: bool = False, fused_item: bool = False,
                 fused_player: bool = False, fused_decoder: bool = False, seed: int = 0, query_scale: float = 1.0):
        super().__init__()
        self._calling(task_dim, fused_heads, fused_decoder, seed, query_scale)

        self.tile_encoder = TileEncoder(hidden, fused=fused_tile, fused_conv2=fused_tile_conv2)
        self.player_encoder = PlayerEncoder(hidden, hidden, fused=fused_player)
        self.item_encoder = ItemEncoder(hidden, fused=fused_item)
        self.inventory_encoder = _Fc(layout.INVENTORY_N_OBS * hidden, hidden)
        self.market_encoder = _Fc(hidden, hidden)
        self.task_encoder = _Fc(task_dim, hidden)
        self.proj_fc = nn.Linear(6 * hidden, hidden)
        self.action_decoder = ActionDecoder(hidden, self.dims)
        self.value_head = nn.Linear(hidden, 1)

    def _calling(self, task_dim: int, fused_heads: bool, fused_decoder: bool, seed: int, query_scale: float):
        """What `decode_actions` and `masked` need besides the modules: the sampling state and where the
        sections, masks and heads lie in an obs row. (`reduced.ReducedAgent` shares it.)"""
        self.fused_heads, self.fused_decoder = bool(fused_heads), bool(fused_decoder)
        self.seed = int(seed)
        self.draws = 0  # sampling calls so far: the `offset` of the next one
        self.query_scale = float(query_scale)  # 1.0 is the reference's; the stand-ins use 1 / sqrt(hidden)
        lay = layout.flat_layout(task_dim)
        self.task_dim = int(task_dim)
        self.o_tile, self.o_id, self.o_task = lay["Tile"].offset, lay["AgentId"].offset, lay["Task"].offset
        self.sections = {name: (lay[name].offset, *lay[name].shape) for name in SETS}
        self.dims = list(layout.ACTION_DIMS)
        self.mask_off = np.cumsum([0] + self.dims).tolist()
        self.head_set = [-1 if s is None else SETS.index(s) for _, s in DECODER_LAYERS]
        for k, (_, s) in enumerate(DECODER_LAYERS):
            assert s is None or self.dims[k] == self.sections[s][1] + 1, (k, s)
        self.pointer = [k for k, s in enumerate(self.head_set) if s >= 0]  # in head order: pq's slots
        self.set_heads = [[k for k in self.pointer if self.head_set[k] == s] for s in range(len(SETS))]

    # ---------------------------------------------------------------- views of the obs rows
    def section(self, obs: torch.Tensor, name: str) -> torch.Tensor:
        """The rows' Entity, Inventory or Market section [N, rows * cols], a view of `obs`."""
        o, rows, cols = self.sections[name]
        return obs[:, o:o + rows * cols]

    def _embeddings(self, obs: torch.Tensor):
        """{set: [N, R, H]} for the sets whose encoder is not fused: the reference's embeddings."""
        emb = {}
        if not self.player_encoder.fused:
            emb["Entity"] = self.player_encoder.embed(self.section(obs, "Entity"), layout.PLAYER_N_OBS)
        if not self.item_encoder.fused:
            emb["Inventory"] = self.item_encoder.embed(self.section(obs, "Inventory"), layout.INVENTORY_N_OBS)
            emb["Market"] = self.item_encoder.embed(self.section(obs, "Market"), layout.MARKET_N_OBS)
        return emb

    # ---------------------------------------------------------------- encoder
    def _encode(self, obs: torch.Tensor):
        emb = self._embeddings(obs)
        penc, ienc = self.player_encoder, self.item_encoder
        ents, inv, mk = (self.section(obs, name) for name in SETS)
        tile = self.tile_encoder(obs, self.o_tile)
        my_agent = penc.my_agent(ents, obs[:, self.o_id], layout.PLAYER_N_OBS)
        if penc.fused:
            players = penc.pooled(ents, layout.PLAYER_N_OBS)
        else:
            players = emb["Entity"].mean(1)
        if ienc.fused:  # a linear layer and a mean commute
            items = ienc.pooled(inv, layout.INVENTORY_N_OBS)
            market = self.market_encoder.fc(ienc.pooled(mk, layout.MARKET_N_OBS))
        else:
            items = emb["Inventory"].mean(1)
            market = self.market_encoder.fc(emb["Market"]).mean(-2)
        task = self.task_encoder.fc(obs[:, self.o_task:self.o_task + self.task_dim])
        return self.proj_fc(torch.cat([tile, my_agent, players, items, market, task], -1)), emb

    def encode_observations(self, obs: torch.Tensor) -> torch.Tensor:
        """The hidden rows [N, hidden]: the reference's `encode_observations` without its lookup, which
        `decode_actions` takes from the obs rows."""
        return self._encode(obs)[0]

    # ---------------------------------------------------------------- decoder
    def decode_actions(self, hidden: torch.Tensor, obs: torch.Tensor, action: torch.Tensor | None = None, emb=None,
                       greedy: bool = False):
        """(action, logprob, entropy, value) of the hidden rows `hidden` of the rows `obs`. `greedy`:
        select every head's first maximal legal entry instead of sampling (see `masked`)."""
        if greedy and action is not None:
            raise ValueError("greedy=True selects the actions: it cannot be combined with action=")
        layers = self.action_decoder.layers
        out = [layers[name](hidden) for name, _ in DECODER_LAYERS]
        dense = [out[k] for k, s in enumerate(self.head_set) if s < 0]
        queries = {k: out[k] * self.query_scale if self.query_scale != 1.0 else out[k] for k in self.pointer}
        value = self.value_head(hidden)
        if self.fused_decoder:
            from .decoder import decoder_heads

            sets = [(self.section(obs, "Entity"), "entity"), (self.section(obs, "Inventory"), "item"),
                    (self.section(obs, "Market"), "item")]
            acts, logp, ent = decoder_heads(torch.cat(dense, 1), self.pointer_slots(queries), sets, self.head_set, obs,
                                            self.dims, action, seed=self.seed, offset=self.draws, greedy=greedy)
            if action is None and not greedy:
                self.draws += 1
            return acts, logp, ent, value
        return (*self.masked(self.logits(out, queries, obs, emb), obs, action, greedy), value)

    def pointer_slots(self, queries) -> torch.Tensor:
        """pq [N, 8, 40]: the pointer heads' queries folded into the encoders' first layers, one
        40-float slot per pointer head in head order (an item head's 36 floats padded with zeros)."""
        slots = {**self._fold(queries, "Entity"), **self._fold(queries, "Inventory")}
        return torch.stack([slots[k] for k in self.pointer], 1)

    def _fold(self, queries, name: str) -> dict:
        """{head: its slot [N, 40]} for the heads over `name`'s encoder: the three entity heads, or the
        five heads of the two item sets, which share the item encoder and are folded by one product
        whichever path asks (so the fused decoder and the composed path see the same bits)."""
        if name == "Entity":
            ks = self.set_heads[SETS.index("Entity")]
            pq = self.player_encoder.pointer_query(torch.stack([queries[k] for k in ks], 1))
        else:
            ks = self.set_heads[SETS.index("Inventory")] + self.set_heads[SETS.index("Market")]
            pq = self.item_encoder.pointer_query(torch.stack([queries[k] for k in ks], 1))
            pq = torch.cat([pq, pq.new_zeros(*pq.shape[:-1], 40 - pq.shape[-1])], -1)
        return {k: pq[:, i] for i, k in enumerate(ks)}

    def logits(self, out, queries, obs: torch.Tensor, emb=None) -> torch.Tensor:
        """The twelve heads' logits [N, 1586] in head order: a fused encoder's pointer heads through
        `item_logits` / `player_logits` (their illegal and no-op entries are 0), the others the
        reference's way, a zero row appended to the embeddings and `matmul`."""
        if emb is None:
            emb = self._embeddings(obs)
        parts = list(out)
        slots = {}
        for s, name in enumerate(SETS):
            ks = self.set_heads[s]
            width = self.sections[name][1] + 1
            enc = self.player_encoder if name == "Entity" else self.item_encoder
            if enc.fused:
                lg = self._set_logits(name, ks, queries, obs, slots)
                for i, k in enumerate(ks):
                    parts[k] = lg[:, i * width:(i + 1) * width]
            else:
                e = emb[name]
                padded = torch.cat([e, e.new_zeros(e.shape[0], 1, e.shape[2])], 1)
                for k in ks:
                    parts[k] = torch.matmul(padded, queries[k].unsqueeze(-1)).squeeze(-1)
        return torch.cat(parts, 1)

    def _set_logits(self, name: str, ks, queries, obs: torch.Tensor, slots: dict) -> torch.Tensor:
        """[N, len(ks) * (R + 1)]: the heads `ks` over set `name` from its fused encoder's kernel. `slots`
        keeps the folded queries between the two item sets of one `logits` call."""
        from .item import QUERY as ITEM_QUERY, item_logits
        from .player import QUERY as PLAYER_QUERY, player_logits

        if ks[0] not in slots:
            slots.update(self._fold(queries, name))
        pq = torch.stack([slots[k][:, :PLAYER_QUERY if name == "Entity" else ITEM_QUERY] for k in ks], 1)
        fn = player_logits if name == "Entity" else item_logits
        return fn(self.section(obs, name), pq, obs, [self.mask_off[k] for k in ks], set_rows=self.sections[name][1])

    def masked(self, logits: torch.Tensor, obs: torch.Tensor, action: torch.Tensor | None = None,
               greedy: bool = False):
        """(action, logprob, entropy) of the heads' concatenated logits under the rows' ActionTargets.
        `greedy` replaces the draw by the argmax of the masked logits, ties to the smallest index
        (SPEC.md §24; what an evaluation run wants): deterministic, and `draws` does not advance."""
        if greedy and action is not None:
            raise ValueError("greedy=True selects the actions: it cannot be combined with action=")
        if self.fused_heads:
            from .heads import masked_heads

            acts, logp, ent = masked_heads(logits, obs, self.dims, action, seed=self.seed, offset=self.draws,
                                           greedy=greedy)
            if action is None and not greedy:
                self.draws += 1
            return acts, logp, ent
        masks = obs[:, :self.mask_off[-1]] > 0
        acts, logp, ent = [], 0.0, 0.0
        for k in range(len(self.dims)):
            lo, hi = self.mask_off[k], self.mask_off[k + 1]
            filled = logits[:, lo:hi].masked_fill(~masks[:, lo:hi], -1e9)
            dist = torch.distributions.Categorical(logits=filled)
            if greedy:
                a = filled.argmax(-1)  # the first maximum
            else:
                a = dist.sample() if action is None else action[:, k]
            acts.append(a)
            logp = logp + dist.log_prob(a)
            ent = ent + dist.entropy()
        return torch.stack(acts, 1), logp, ent

    def forward(self, obs: torch.Tensor, action: torch.Tensor | None = None, greedy: bool = False):
        hidden, emb = self._encode(obs)
        return self.decode_actions(hidden, obs, action, emb, greedy)


class RecurrentBaselineAgent(nn.Module):
    """The policy the start kit trains and evaluates, `Recurrent(Baseline)` (train.py:65-71,
    evaluate.py:98-105, config.yaml:93-96): an LSTM between `encode_observations` and `decode_actions`.

        agent = RecurrentBaselineAgent(task_dim, hidden=256, fused_lstm=True, fused_decoder=True).cuda()
        action, logprob, entropy, value, state = agent(obs, state)              # sample, one step
        _, logprob, entropy, value, state = agent(window, state, action=action)  # evaluate a bptt window
        action, *_ = agent(obs, state, greedy=True)                              # select, for scoring

    The submodules carry the names pufferlib's wrapper gives them, `policy` (a `BaselineAgent`, which
    takes every keyword this class does not name) and `recurrent` (`lstm.LSTM`, SPEC.md §17, with
    `fused_lstm`, else `torch.nn.LSTM`; both time-first), so that a start-kit checkpoint's
    `state_dict`, keys `policy.*` and `recurrent.{weight_ih,weight_hh,bias_ih,bias_hh}_l{k}`, loads
    whole with `strict=True` under either flag. `lstm` is `recurrent` under the name `DeviceTrainer`
    looks for; it is a property, not a second registration. `recurrent` starts as the wrapper's does
    [recalled: pufferlib 0.7.3 `RecurrentWrapper.__init__`, which is not importable here]: biases 0,
    weights orthogonal with gain 1.0. `seed`, `draws` and `query_scale` are `policy`'s.

    The calling convention is the wrapper's and `trainer.RecurrentMaskedAgent`'s: obs is [B, E] (one
    step) or [B, T, E] (a window), the four outputs are flattened in (B, T) order, state is (h, c),
    each [num_layers, B, hidden], or None for zeros. Under `torch.no_grad()` with `fused_lstm` a given
    state is updated in place and returned."""

    POLICY = BaselineAgent  # what `policy` is: `reduced.RecurrentReducedAgent` names another

    def __init__(self, task_dim: int = 2048, hidden: int = 256, num_layers: int = 1, fused_lstm: bool = False,
                 **baseline_flags):
        super().__init__()
        self.fused_lstm = bool(fused_lstm)
        self.policy = self.POLICY(task_dim, hidden=hidden, **baseline_flags)
        if self.fused_lstm:
            from .lstm import LSTM

            self.recurrent = LSTM(hidden, hidden, num_layers)  # hidden: a multiple of 64, or a ValueError
        else:
            self.recurrent = nn.LSTM(hidden, hidden, num_layers)
        for name, p in self.recurrent.named_parameters():
            if "bias" in name:
                nn.init.constant_(p, 0.0)
            else:
                nn.init.orthogonal_(p, 1.0)

    @property
    def lstm(self):
        return self.recurrent

    seed = property(lambda self: self.policy.seed, lambda self, v: setattr(self.policy, "seed", int(v)))
    draws = property(lambda self: self.policy.draws, lambda self, v: setattr(self.policy, "draws", int(v)))
    query_scale = property(lambda self: self.policy.query_scale,
                           lambda self, v: setattr(self.policy, "query_scale", float(v)))

    def forward(self, obs: torch.Tensor, state=None, action: torch.Tensor | None = None, greedy: bool = False):
        B, T = obs.shape[0], (obs.shape[1] if obs.dim() == 3 else 1)
        flat = obs.reshape(B * T, obs.shape[-1])  # rows in (B, T) order; a view of a contiguous obs
        hidden, emb = self.policy._encode(flat)
        x = hidden.view(B, T, -1).transpose(0, 1)  # time first
        if self.fused_lstm and state is not None and not torch.is_grad_enabled():
            y, state = self.recurrent(x, state, out=state)
        else:
            y, state = self.recurrent(x, state)
        hidden = y.transpose(0, 1).reshape(B * T, -1)
        if action is not None:
            action = action.reshape(B * T, -1)
        return (*self.policy.decode_actions(hidden, flat, action, emb, greedy), state)
