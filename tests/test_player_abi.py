"""The player-encoder entry points of libnmmo_heads.so (include/nmmo_heads.h, SPEC.md §21) and
nmmo_amd/player.py without a GPU: the constants match the header as a C compiler reads it, every
argument rule is refused with NMH_E_INVALID and a message naming the field (every call passes dummy
non-null pointers and n = 0, so a missing check shows as NMH_OK, never as a launch),
`player_features_ref` is the reference's lines 124-130, `own_row_ref` its lines 132-140, and in
float64 the pooled embedding, the projected-query logits and my_agent equal the materialised chain
(embed, pad, matmul, mean, gather). CPU only."""

import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from nmmo_amd import heads, player

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = 0x1000  # non-null, 16-byte aligned, never dereferenced


def test_constants_match_the_c_compiler():
    src = r"""
#include <stdio.h>
#include <stddef.h>
#include "nmmo_heads.h"
int main(void) {
  printf("%d %d %d %d %d %d %d %d %d %d %d\n", NMH_PLAYER_COLS, NMH_PLAYER_FEATURES, NMH_PLAYER_QUERY,
         NMH_PLAYER_MAX_ROWS, NMH_PLAYER_MAX_HEADS, NMH_PLAYER_TYPES, NMH_PLAYER_F32, NMH_PLAYER_I16,
         (int)sizeof(NmhPlayerHeads), (int)offsetof(NmhPlayerHeads, mask_off), (int)offsetof(NmhPlayerHeads, out_off));
  return 0;
}
"""
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        with open(c, "w") as fh:
            fh.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [player.COLS, player.FEATURES, player.QUERY, player.MAX_ROWS, player.MAX_HEADS, player.TYPES,
                   player.PLAYER_F32, player.PLAYER_I16, ctypes.sizeof(player.NmhPlayerHeads),
                   player.NmhPlayerHeads.mask_off.offset, player.NmhPlayerHeads.out_off.offset]
    assert got == [31, 35, 40, 256, 4, 5, 0, 1, 36, 4, 20]
    assert (player.ID_COL, player.TYPE_COL) == (0, 1)


class Args:
    """Valid arguments with no rows; a test bends one of them."""

    def __init__(self, set_rows=100, n_heads=3):
        self.n = 0
        self.ents, self.ent_stride, self.kind, self.set_rows = DUMMY, 31 * set_rows, player.PLAYER_F32, set_rows
        self.ids, self.id_stride, self.id_kind = DUMMY, 1, player.PLAYER_F32
        self.features = self.sums = self.mine = self.mine_idx = DUMMY
        self.mask = self.pq = self.out = self.g_out = self.g_pq = DUMMY
        self.mask_kind = heads.MASK_F32
        width = set_rows + 1
        self.ph = player.player_heads_struct([7 + h * width for h in range(n_heads)],
                                             [h * width for h in range(n_heads)])
        self.mask_stride, self.out_stride = 7 + n_heads * width, n_heads * width

    def features_(self):
        return heads.lib().nmh_player_features(self.n, self.ents, self.ent_stride, self.kind, self.set_rows, self.ids,
                                               self.id_stride, self.id_kind, self.features, self.sums, self.mine,
                                               self.mine_idx, None)

    def logits(self):
        return heads.lib().nmh_player_logits(ctypes.byref(self.ph), self.n, self.ents, self.ent_stride, self.kind,
                                             self.set_rows, self.mask, self.mask_stride, self.mask_kind, self.pq,
                                             self.out, self.out_stride, None)

    def logits_backward(self):
        return heads.lib().nmh_player_logits_backward(
            ctypes.byref(self.ph), self.n, self.ents, self.ent_stride, self.kind, self.set_rows, self.mask,
            self.mask_stride, self.mask_kind, self.g_out, self.out_stride, self.g_pq, None)


FNS = {"features": "features_", "logits": "logits", "logits_backward": "logits_backward"}


def refused(a, fn, *words):
    rc = getattr(a, FNS[fn])()
    msg = heads.lib().nmh_last_error().decode()
    assert rc == heads.NMH_E_INVALID, (fn, rc, msg)
    assert msg.startswith(f"nmh_player_{fn}:"), msg
    for w in words:
        assert w in msg, (fn, w, msg)


def test_valid_arguments_with_no_rows_are_a_no_op():
    for a in (Args(), Args(1, 1), Args(256, 1), Args(256, 4)):
        assert a.features_() == a.logits() == a.logits_backward() == heads.NMH_OK
        a.kind, a.id_kind, a.mask_kind = player.PLAYER_I16, player.PLAYER_I16, heads.MASK_U8
        a.ent_stride = a.id_stride = 23987
        assert a.features_() == a.logits() == a.logits_backward() == heads.NMH_OK
        for keep in ("features", "sums", "mine", "mine_idx"):  # any output alone
            a.features = a.sums = a.mine = a.mine_idx = None
            setattr(a, keep, DUMMY)
            assert a.features_() == heads.NMH_OK, keep
        a.features, a.sums, a.mine, a.mine_idx, a.ids = DUMMY, DUMMY, None, None, None  # no own row: no ids
        a.id_kind, a.id_stride = 9, 0  # ... and nothing about them is looked at
        assert a.features_() == heads.NMH_OK


@pytest.mark.parametrize("fn", sorted(FNS))
def test_bad_kind_rows_and_stride_are_refused(fn):
    for kind in (2, -1):
        a = Args()
        a.kind = kind
        refused(a, fn, "ent_kind", str(kind))
    for rows in (0, 257, -1):
        a = Args()
        a.set_rows, a.ent_stride, a.mask_stride, a.out_stride = rows, 1 << 20, 1 << 20, 1 << 20
        refused(a, fn, "set_rows", str(rows))
    a = Args(100)
    a.ent_stride = 31 * 100 - 1
    refused(a, fn, "ent_stride", "3099")
    a = Args()
    a.ents = None
    refused(a, fn, "ents", "NULL")
    a = Args()
    a.n = -1
    refused(a, fn, "n_sets" if fn == "features" else "n_rows", "-1")


def test_features_without_an_output_or_without_ids_are_refused():
    a = Args()
    a.features = a.sums = a.mine = a.mine_idx = None
    refused(a, "features", "features", "sums", "mine", "mine_idx", "NULL")
    for keep in ("mine", "mine_idx"):
        a = Args()
        a.features = a.sums = a.mine = a.mine_idx = a.ids = None
        setattr(a, keep, DUMMY)
        refused(a, "features", "ids", "NULL")
    for kind in (2, -1):
        a = Args()
        a.id_kind = kind
        refused(a, "features", "id_kind", str(kind))
    for stride in (0, -5):
        a = Args()
        a.id_stride = stride
        refused(a, "features", "id_stride", str(stride))


@pytest.mark.parametrize("fn", ["logits", "logits_backward"])
def test_bad_heads_strides_and_pointers_are_refused(fn):
    for n_heads in (0, 5, -1):
        a = Args()
        a.ph.n_heads = n_heads
        refused(a, fn, "n_heads", str(n_heads))
    a = Args(12, 4)  # the furthest head ends at 3 * 13 + 13 = 52
    a.out_stride = 51
    refused(a, fn, "out_stride" if fn == "logits" else "g_stride", "51")
    a.out_stride = 52
    assert getattr(a, fn)() == heads.NMH_OK
    a.ph.out_off[1] = 40  # heads need not be in order: the furthest counts
    refused(a, fn, "out_stride" if fn == "logits" else "g_stride", "52")
    a = Args(12, 4)
    a.mask_stride -= 1
    refused(a, fn, "mask_stride", str(a.mask_stride))
    a = Args()
    a.ph.mask_off[2] = -1
    refused(a, fn, "mask_off")
    a = Args()
    a.mask_kind = 2
    refused(a, fn, "mask_kind", "2")
    for field in ("mask", "pq", "out") if fn == "logits" else ("mask", "g_out", "g_pq"):
        a = Args()
        setattr(a, field, None)
        refused(a, fn, field, "NULL")
    rc = getattr(heads.lib(), f"nmh_player_{fn}")(None, 0, DUMMY, 3100, 0, 100, DUMMY, 999, 0, DUMMY, *(
        (DUMMY, 999, None) if fn == "logits" else (999, DUMMY, None)))
    assert rc == heads.NMH_E_INVALID and b"ph is NULL" in heads.lib().nmh_last_error()


def test_misaligned_pq_is_refused():
    a = Args()
    a.pq = DUMMY + 4
    refused(a, "logits", "pq", "16-byte")
    a = Args()
    a.out = a.ents = a.mask = DUMMY + 4  # nothing else needs more than its element's alignment
    a.g_out = a.g_pq = a.ids = a.features = a.sums = a.mine = a.mine_idx = DUMMY + 4
    assert a.logits() == heads.NMH_OK and a.logits_backward() == heads.NMH_OK and a.features_() == heads.NMH_OK


# ---------------------------------------------------------------- nmmo_amd/player.py
def reference_features(agents):
    """baseline_policy.py:124-130, literally (one_hot raises outside the classes)."""
    npc_type = agents[:, :, 1]
    one_hot_npc_type = F.one_hot(npc_type.long(), num_classes=5).float()
    return torch.cat([agents[:, :, :1], one_hot_npc_type, agents[:, :, 2:]], dim=-1).float()


def reference_own_row(one_hot_agents, my_id):
    """baseline_policy.py:132-140, literally (EntityId is column 0)."""
    agent_ids = one_hot_agents[:, :, 0]
    mask = (agent_ids == my_id.unsqueeze(1)) & (agent_ids != 0)
    mask = mask.int()
    row_indices = torch.where(mask.any(dim=1), mask.argmax(dim=1), torch.zeros_like(mask.sum(dim=1)))
    return one_hot_agents[torch.arange(one_hot_agents.shape[0]), row_indices], row_indices


def sample_ents(n, rows, rng):
    """[n, rows, 31] float32 entity sets with integer values: about half the rows empty, distinct
    non-zero ids (players positive, NPCs negative), every npc_type."""
    x = rng.integers(-200, 2000, (n, rows, 31)).astype(np.float32)
    ids = np.stack([rng.permutation(np.arange(1, rows + 1)) for _ in range(n)]).astype(np.float32)
    x[:, :, 0] = np.where(rng.random((n, rows)) < 0.3, -ids, ids)
    x[:, :, 1] = rng.integers(0, 5, (n, rows))
    x[rng.random((n, rows)) < 0.5] = 0
    return torch.from_numpy(x)


def test_player_features_ref_is_the_references_lines_where_those_are_defined():
    x = sample_ents(5, 12, np.random.default_rng(0))
    got = player.player_features_ref(x)
    assert got.dtype == torch.float32 and got.shape == (5, 12, 35)
    assert torch.equal(got, reference_features(x))
    assert torch.equal(got, torch.cat([x[..., :1], F.one_hot(x[..., 1].long(), 5).float(), x[..., 2:]], -1))
    assert torch.equal(player.player_features_ref(x.to(torch.int16)), got)
    assert torch.equal(player.player_features_ref(x.reshape(60, 31)), got.reshape(60, 35))
    d = player.player_features_ref(x.double())
    assert d.dtype == torch.float64 and torch.equal(d, got.double())


def test_player_features_ref_clamps_where_one_hot_would_raise():
    x = sample_ents(3, 4, np.random.default_rng(1))
    x[0, 0, 1], x[0, -1, 1], x[-1, 0, 1] = -3, 7, np.nan
    with pytest.raises(RuntimeError):
        reference_features(x)
    f = player.player_features_ref(x)
    assert f[0, 0, 1:6].argmax() == 0 and f[0, -1, 1:6].argmax() == 4 and f[-1, 0, 1] == 1  # -3 -> 0, 7 -> 4, NaN -> 0
    assert torch.equal(f[..., 1:6].sum(-1), torch.ones(3, 4))
    keep = [0] + list(range(6, 35))
    assert torch.equal(f[..., keep], x[..., [0] + list(range(2, 31))])  # the other columns pass through raw


def test_own_row_ref_is_the_references_lines():
    R = 6
    x = torch.zeros((7, R, 31))
    x[..., 2] = torch.arange(7 * R).reshape(7, R).float() + 1  # tells the rows apart
    ids = torch.tensor([5.0, 9.0, 4.0, 8.0, 0.0, -3.0, float("nan")])
    x[0, 0, 0] = 5                    # a match at row 0
    x[0, 3, 0] = 2
    x[1, R - 1, 0] = 9                # a match at row R - 1
    x[2, 2, 0] = x[2, 4, 0] = 4       # two matches: the first wins
    x[2, 0, 0] = 1
    x[3, :, 0] = torch.arange(1, R + 1).float()  # no match
    x[4, 1, 0] = 3                    # id 0 among zero-id rows: 0, not the first zero-id row after a non-zero one
    x[5, 1, 0], x[5, 2, 0] = 3, -3    # a negative NPC id
    x[6, :, 0] = float("nan")         # a NaN id matches nothing, not even NaN
    mine, idx = player.own_row_ref(x, ids)
    assert idx.tolist() == [0, R - 1, 2, 0, 0, 2, 0] and idx.dtype == torch.int64
    feats = player.player_features_ref(x)
    assert torch.equal(mine[:6], feats[torch.arange(6), idx[:6]])
    want_mine, want_idx = reference_own_row(feats, ids)
    assert torch.equal(idx, want_idx) and torch.equal(mine[:6], want_mine[:6])
    # int16 entities and ids, ids as [N, 1]
    mine16, idx16 = player.own_row_ref(x[:6].to(torch.int16), ids[:6].to(torch.int16).reshape(6, 1))
    assert torch.equal(idx16, idx[:6]) and torch.equal(mine16, mine[:6])
    rng = np.random.default_rng(4)
    y = sample_ents(9, 100, rng)
    yid = y[torch.arange(9), torch.from_numpy(rng.integers(0, 100, 9)), 0].clone()  # about half of them empty rows'
    got, want = player.own_row_ref(y, yid), reference_own_row(reference_features(y), yid)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and int((got[1] > 0).sum()) > 0


@torch.no_grad()
def test_pooled_projected_query_logits_and_my_agent_equal_the_materialised_chain_in_float64():
    torch.manual_seed(0)
    rng = np.random.default_rng(2)
    enc = player.PlayerEncoder(20, 24).double()
    for rows in (1, 12, 100):
        x = sample_ents(4, rows, rng).double()
        ids = x[torch.arange(4), torch.tensor([0, rows - 1, rows // 2, 0]), 0].clone()
        ids[3] = 5000.0  # nobody
        q = torch.randn(4, 3, 24, dtype=torch.float64)
        emb = enc.embed(x)  # the reference's chain: embed, pad, matmul, mean, gather
        assert emb.shape == (4, rows, 24)
        padded = torch.cat([emb, emb.new_zeros(4, 1, 24)], 1)
        want = torch.stack([torch.matmul(padded, q[:, h].unsqueeze(-1)).squeeze(-1) for h in range(3)], 1)
        want_pooled = emb.mean(1)
        feats = reference_features(x).double()
        own, idx = reference_own_row(feats, ids)
        want_mine = F.relu(enc.my_agent_fc(own))
        # what the fused path computes: sums / R through agent_fc, pq . (x, 1), my_agent_fc of the own row's x
        f = player.player_features_ref(x)
        pooled = F.linear(f.sum(1) / rows, enc.agent_fc.weight, enc.agent_fc.bias)
        pq = enc.pointer_query(q)
        assert pq.shape == (4, 3, 40) and torch.equal(pq[..., 36:], torch.zeros(4, 3, 4, dtype=torch.float64))
        got = torch.einsum("nhf,njf->nhj", pq[..., :35], f) + pq[..., 35:36]
        scale = max(1.0, float(want.abs().max()))
        assert float((got - want[..., :rows]).abs().max()) <= 1e-12 * scale
        assert torch.equal(want[..., rows], torch.zeros(4, 3, dtype=torch.float64))  # the no-op: the zero row
        assert float((pooled - want_pooled).abs().max()) <= 1e-12 * max(1.0, float(want_pooled.abs().max()))
        assert float((enc.pooled(x) - want_pooled).abs().max()) <= 1e-12 * max(1.0, float(want_pooled.abs().max()))
        mine, got_idx = player.own_row_ref(x, ids)
        assert torch.equal(got_idx, idx)
        got_mine = F.relu(F.linear(mine, enc.my_agent_fc.weight, enc.my_agent_fc.bias))
        assert got_mine.shape == (4, 20)
        assert float((got_mine - want_mine).abs().max()) <= 1e-12 * max(1.0, float(want_mine.abs().max()))
        assert float((enc.my_agent(x, ids) - want_mine).abs().max()) <= 1e-12 * max(1.0, float(want_mine.abs().max()))
        assert torch.equal(enc.my_agent(x.reshape(4, -1), ids.reshape(4, 1), set_rows=rows), enc.my_agent(x, ids))


def test_player_encoder_parameter_names_are_the_references():
    for fused in (False, True):
        sd = player.PlayerEncoder(256, 128, fused=fused).state_dict()
        assert {k: tuple(v.shape) for k, v in sd.items()} == {
            "agent_fc.weight": (128, 35), "agent_fc.bias": (128,), "my_agent_fc.weight": (256, 35),
            "my_agent_fc.bias": (256,)}
    a, b = player.PlayerEncoder(32, 32), player.PlayerEncoder(32, 32, fused=True)
    b.load_state_dict(a.state_dict())
    a.load_state_dict(b.state_dict())


def test_host_tensors_are_refused_without_a_fallback():
    enc = player.PlayerEncoder(32, 32, fused=True)
    x, ids = torch.zeros((2, 100, 31)), torch.zeros(2)
    for call in (lambda: player.player_features(x), lambda: player.player_sums(x), lambda: player.player_own(x, ids),
                 lambda: enc.embed(x), lambda: enc.pooled(x), lambda: enc.my_agent(x, ids),
                 lambda: player.player_logits(x, torch.zeros(2, 1, 40), torch.ones(2, 101), [0])):
        with pytest.raises(heads.HeadsError, match="GPU"):
            call()


def test_player_agent_defaults_to_unfused_and_keeps_the_stand_ins_call_convention():
    from nmmo_amd import layout
    from nmmo_amd.trainer import PlayerMaskedAgent

    torch.manual_seed(0)
    agent = PlayerMaskedAgent(16, hidden=32)
    assert not agent.player_encoder.fused and not agent.fused_heads
    assert PlayerMaskedAgent(16, hidden=32, fused_player=True).player_encoder.fused
    assert PlayerMaskedAgent(16, hidden=32, fused_heads=True).fused_heads
    assert sum(agent.dims) == 1586 and len(agent.queries) == 3 and len(agent.dense) == 9
    assert [agent.dims[k] for k in agent.target_heads] == [101, 101, 101]
    obs = torch.zeros((3, layout.obs_elems(16)))
    obs[:, :sum(agent.dims)] = 1.0
    ents, ids = agent.entities(obs)
    ents.reshape(3, 100, 31)[:, :5, 0] = torch.tensor([3.0, 7.0, -2.0, 9.0, 1.0])
    ents.reshape(3, 100, 31)[:, :5, 2:] = torch.arange(5 * 29).reshape(5, 29).float() % 13
    ids[:] = torch.tensor([7.0, 1.0, 50.0])
    keep = obs.clone()
    a, logp, ent, value = agent(obs)
    assert torch.equal(obs, keep)
    assert a.shape == (3, len(agent.dims)) and logp.shape == ent.shape == (3,) and value.shape == (3, 1)
    _, logp2, _, _ = agent(obs, action=a)
    assert torch.allclose(logp, logp2)
    h, emb = agent.hidden(obs)
    assert emb.shape == (3, 100, 32) and not torch.equal(h[0], h[1]) and not torch.equal(h[0], h[2])  # the own row
    assert {n.split(".")[0] for n, _ in agent.named_parameters()} == {
        "encoder", "player_encoder", "players", "my_agent", "queries", "dense", "value"}
    assert {k for k in agent.state_dict() if k.startswith("player_encoder.")} == {
        "player_encoder.agent_fc.weight", "player_encoder.agent_fc.bias", "player_encoder.my_agent_fc.weight",
        "player_encoder.my_agent_fc.bias"}
