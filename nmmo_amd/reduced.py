"""The takeru `ReducedModelV2` policy (agent_zoo/takeru/policy.py:21-405) assembled from this package's
modules: five encoders into `proj_fc`, the twelve decoder layers and a value head, with the
reference's parameter names and shapes, so that a takeru (or `hybrid`: the same policy under
yaofeng's rewards) policy `state_dict` loads with `strict=True`. The reference keeps its offsets and
scales as plain attributes, not buffers, so the `state_dict` has none of them.

    agent = ReducedAgent(task_dim, fused_tile=True, fused_tile_conv2=True, fused_player=True,
                         fused_item=True, fused_heads=True).cuda()
    action, logprob, entropy, value = agent(obs)                 # sample
    _, logprob, entropy, value = agent(obs, action=action)       # evaluate
    action, logprob, entropy, value = agent(obs, greedy=True)    # select: every head's first maximum

The calling convention, `seed`, `draws` and `query_scale` are `baseline.BaselineAgent`'s, whose decoder
and masked heads this class runs. What differs from the start-kit policy:

- Entity and item rows are embedding lookups, not one-hot features (`embed.ReducedPlayerEncoder`,
  `embed.ReducedItemEncoder`, SPEC.md §25). With `fused_player` / `fused_item` the pointer logits come
  from `embed.embed_logits`, the Market pool from bin counts, and no [N, R, H] tensor exists for Entity
  or Market; the 12 Inventory rows' [N, 12, H] is made either way, because `inventory_encoder.fc` takes
  it flattened.
- The tile encoder embeds the material column alone (`ReducedTileEncoder`).
- `proj_fc` takes tile, my_agent, inventory, market and task, each `input_size` wide, and no pooled
  entity feature; there is no ReLU behind it.

There is no one-launch decoder for this policy (`fused_decoder`): `nmh_decoder_*` knows §20's and §21's
feature rules only.
"""

from __future__ import annotations

import torch
from torch import nn
from torch.nn import functional as F

from . import layout, tile
from .baseline import ActionDecoder, BaselineAgent, RecurrentBaselineAgent, _Fc
from .embed import ReducedItemEncoder, ReducedPlayerEncoder, embed_logits

MATERIAL = 2  # the Tile column the reference keeps (`tile[:, :, 2:]`)
CHANNELS1 = 16  # tile_conv_1's output channels; the kernels' first convolution has tile.CHANNELS = 32


class ReducedTileEncoder(nn.Module):
    """The reference's ReducedTileEncoder (takeru/policy.py:85-112), parameter names and shapes
    included: `embedding [256, 32]` over the material column, `tile_conv_1` 32 -> 16, `tile_conv_2`
    16 -> 8, `tile_fc`. `forward(obs, offset)` as `tile.TileEncoder`'s; the rows are never written.

    `fused=True` and `fused_conv2=True` go through `tile.tile_conv1` / `tile.tile_conv12` (SPEC.md §19,
    §22), whose table is [3, 256, 9, 32]: this policy's [256, 9, 16] table is padded with zeros (the
    row and column features' rows, channels 16..31), so are `tile_conv_1`'s bias and `tile_conv_2`'s
    input channels, and autograd slices the gradients back. The padded terms add +0.0 and the padded
    channels are relu(0) = 0, so the result is the unpadded one; the kernel does about 6 x the lookups
    a kernel written for this table would (3 features x 2 in channels)."""

    def __init__(self, input_size: int, fused: bool = False, fused_conv2: bool = False):
        super().__init__()
        if fused_conv2 and not fused:
            raise ValueError("fused_conv2=True extends the fused path: it needs fused=True")
        self.fused, self.fused_conv2 = bool(fused), bool(fused_conv2)
        self.embedding = nn.Embedding(tile.VALUES, tile.EMBED)
        self.tile_conv_1 = nn.Conv2d(tile.EMBED, CHANNELS1, 3)
        self.tile_conv_2 = nn.Conv2d(CHANNELS1, tile.CHANNELS2, 3)
        self.tile_fc = nn.Linear(tile.CHANNELS2 * tile.OUT2_SIDE * tile.OUT2_SIDE, input_size)

    def padded(self):
        """(table [3, 256, 9, 32], bias1 [32], weight2 [8, 32, 3, 3]) for the kernels; differentiable."""
        w1 = self.tile_conv_1.weight.reshape(CHANNELS1, tile.EMBED, tile.TAPS)
        t = torch.einsum("oek,ve->vko", w1, self.embedding.weight)  # [256, 9, 16]
        t = F.pad(t, (0, tile.CHANNELS - CHANNELS1))
        table = torch.cat([t.new_zeros(MATERIAL, *t.shape), t.unsqueeze(0)], 0).contiguous()
        bias1 = F.pad(self.tile_conv_1.bias, (0, tile.CHANNELS - CHANNELS1))
        weight2 = F.pad(self.tile_conv_2.weight, (0, 0, 0, 0, 0, tile.CHANNELS - CHANNELS1))
        return table, bias1, weight2

    def forward(self, obs: torch.Tensor, offset: int = 0) -> torch.Tensor:
        if obs.dim() == 3:  # [N, 225, 3]: a view when contiguous
            obs = obs.reshape(obs.shape[0], -1)
        x = obs[:, offset:offset + tile.ROW]  # a view: no [N, 225, 3] copy
        if self.fused_conv2:
            table, bias1, weight2 = self.padded()
            t = tile.tile_conv12(x, table, bias1, weight2, self.tile_conv_2.bias)
        else:
            if self.fused:
                table, bias1, _ = self.padded()
                t = tile.tile_conv1(x, table, bias1)[:, :CHANNELS1]
            else:
                t = self.embedding(tile.tile_indices(x)[:, :, MATERIAL])  # [N, 225, 32]
                t = t.transpose(1, 2).reshape(t.shape[0], tile.EMBED, tile.SIDE, tile.SIDE)
                t = F.relu(self.tile_conv_1(t))
            t = F.relu(self.tile_conv_2(t))
        return F.relu(self.tile_fc(t.reshape(t.shape[0], -1)))


class ReducedAgent(BaselineAgent):
    """`ReducedModelV2` (see the module's text). A `BaselineAgent` in everything that follows the
    encoders, the layout of an obs row, `decode_actions`, `masked` and `forward`, with its own modules,
    `_encode` and the fused sets' logits."""

    def __init__(self, task_dim: int = 2048, input_size: int = 256, hidden: int = 256, *, fused_tile: bool = False,
                 fused_tile_conv2: bool = False, fused_player: bool = False, fused_item: bool = False,
                 fused_heads: bool = False, seed: int = 0, query_scale: float = 1.0):
        nn.Module.__init__(self)
        self._calling(task_dim, fused_heads, False, seed, query_scale)
        self.tile_encoder = ReducedTileEncoder(input_size, fused=fused_tile, fused_conv2=fused_tile_conv2)
        self.player_encoder = ReducedPlayerEncoder(input_size, hidden, fused=fused_player)
        self.item_encoder = ReducedItemEncoder(input_size, hidden, fused=fused_item)
        self.inventory_encoder = _Fc(layout.INVENTORY_N_OBS * hidden, input_size)
        self.market_encoder = _Fc(hidden, input_size)
        self.task_encoder = _Fc(task_dim, input_size)
        self.proj_fc = nn.Linear(5 * input_size, hidden)
        self.action_decoder = ActionDecoder(hidden, self.dims)
        self.value_head = nn.Linear(hidden, 1)

    def _embeddings(self, obs: torch.Tensor):
        """{set: [N, R, H]}: the Inventory's always, Entity's and Market's where their encoder is not fused."""
        emb = {"Inventory": self.item_encoder.embed(self.section(obs, "Inventory"), layout.INVENTORY_N_OBS)}
        if not self.player_encoder.fused:
            emb["Entity"] = self.player_encoder.embed(self.section(obs, "Entity"), layout.PLAYER_N_OBS)
        if not self.item_encoder.fused:
            emb["Market"] = self.item_encoder.embed(self.section(obs, "Market"), layout.MARKET_N_OBS)
        return emb

    def _encode(self, obs: torch.Tensor):
        emb = self._embeddings(obs)
        tile_out = self.tile_encoder(obs, self.o_tile)
        my_agent = self.player_encoder.my_agent(self.section(obs, "Entity"), obs[:, self.o_id], layout.PLAYER_N_OBS)
        inventory = self.inventory_encoder.fc(emb["Inventory"].flatten(1))
        if self.item_encoder.fused:  # a linear layer and a mean commute
            market = self.market_encoder.fc(self.item_encoder.pooled(self.section(obs, "Market"), layout.MARKET_N_OBS))
        else:
            market = self.market_encoder.fc(emb["Market"]).mean(-2)
        task = self.task_encoder.fc(obs[:, self.o_task:self.o_task + self.task_dim])
        return self.proj_fc(torch.cat([tile_out, my_agent, inventory, market, task], -1)), emb

    def _set_logits(self, name: str, ks, queries, obs: torch.Tensor, slots: dict) -> torch.Tensor:
        """[N, len(ks) * (R + 1)]: the heads `ks` over set `name` through `embed_logits`, their queries
        folded into score tables by the set's encoder."""
        enc = self.player_encoder if name == "Entity" else self.item_encoder
        pq = enc.pointer_query(torch.stack([queries[k] for k in ks], 1))
        return embed_logits(enc.kind, self.section(obs, name), pq, obs, [self.mask_off[k] for k in ks],
                            set_rows=self.sections[name][1])


class RecurrentReducedAgent(RecurrentBaselineAgent):
    """`Recurrent(ReducedModelV2)` with `num_layers = 1`, the `hybrid` configuration: `policy` is a
    `ReducedAgent`, which takes every keyword `RecurrentBaselineAgent` does not name (`input_size` and
    the `fused_*` flags among them), and `recurrent` is the LSTM over `proj_fc`'s `hidden` outputs.
    Calling convention, `state_dict` keys and initialisation are `RecurrentBaselineAgent`'s."""

    POLICY = ReducedAgent
