"""`baseline.RecurrentBaselineAgent`, the start-kit `Recurrent(Baseline)`, greedy action selection on
the unfused path, and the three `*_argmax` entry points of libnmmo_heads.so (include/nmmo_heads.h,
SPEC.md §24), without a GPU: the `state_dict` is pufferlib's wrapper's (`policy.*` + `recurrent.*`), a
forward over [B, E] and [B, T, E] rows is `encode_observations` -> LSTM -> `decode_actions` written out,
in (B, T) order; `greedy=True` is numpy's first argmax over the masked logits and leaves `draws` alone;
and the new symbols refuse bad arguments as their base functions do. CPU only."""

import ctypes
import re

import numpy as np
import pytest
import torch
from torch import nn

from nmmo_amd import heads
from nmmo_amd.baseline import DECODER_LAYERS, BaselineAgent, RecurrentBaselineAgent
from tests import test_decoder_abi, test_pointer_heads_abi
from tests.test_baseline_agent import make_rows
from tests.test_heads_abi import HEADER, NMMO_DIMS

H = 64


# ---------------------------------------------------------------- names
@pytest.mark.parametrize("fused_lstm", [False, True])
@pytest.mark.parametrize("num_layers", [1, 2])
def test_state_dict_is_the_wrappers(num_layers, fused_lstm):
    base = BaselineAgent(64, H).state_dict()
    want = {"policy." + k: tuple(v.shape) for k, v in base.items()}
    for k in range(num_layers):
        want.update({f"recurrent.weight_ih_l{k}": (4 * H, H), f"recurrent.weight_hh_l{k}": (4 * H, H),
                     f"recurrent.bias_ih_l{k}": (4 * H,), f"recurrent.bias_hh_l{k}": (4 * H,)})
    agent = RecurrentBaselineAgent(64, H, num_layers=num_layers, fused_lstm=fused_lstm)
    assert {k: tuple(v.shape) for k, v in agent.state_dict().items()} == want
    assert agent.lstm is agent.recurrent  # a property: `lstm.*` is not registered a second time
    assert (agent.lstm.num_layers, agent.lstm.hidden_size) == (num_layers, H)
    g = torch.Generator().manual_seed(num_layers)
    sd = {k: torch.randn(shape, generator=g) for k, shape in want.items()}
    agent.load_state_dict(sd, strict=True)
    for k, v in agent.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # the same dict loads under the other flag: the two differ in no name
    RecurrentBaselineAgent(64, H, num_layers=num_layers, fused_lstm=not fused_lstm).load_state_dict(sd, strict=True)


def test_recurrent_starts_as_the_wrappers_and_forwards_the_policys_settings():
    agent = RecurrentBaselineAgent(64, H, num_layers=2, seed=5, query_scale=0.125, fused_heads=True)
    for name, p in agent.recurrent.state_dict().items():
        if "bias" in name:
            assert float(p.abs().max()) == 0.0, name
        else:  # orthogonal, gain 1: the [4H, H] matrix has orthonormal columns
            assert torch.allclose(p.t() @ p, torch.eye(H), atol=1e-5), name
    assert (agent.seed, agent.draws, agent.query_scale) == (5, 0, 0.125)
    assert agent.policy.fused_heads and not agent.fused_lstm
    agent.draws = 7
    assert agent.policy.draws == 7
    with pytest.raises(ValueError):  # lstm.LSTM's rule: a multiple of 64
        RecurrentBaselineAgent(64, 32, fused_lstm=True)
    with pytest.raises(AttributeError):
        agent.lstm = None


# ---------------------------------------------------------------- the forward, unfused
B, T = 3, 2


@pytest.fixture(scope="module")
def rows():
    torch.manual_seed(0)
    agent = RecurrentBaselineAgent(64, H, num_layers=2)
    with torch.no_grad():  # biases 0 would hide a dropped bias
        for name, p in agent.recurrent.named_parameters():
            if "bias" in name:
                p.uniform_(-0.1, 0.1)
    obs, legal = make_rows(B * T)
    return agent, obs, legal


def composed(agent, flat, b, t, state, action):
    """`encode_observations` -> time-first `nn.LSTM` -> `decode_actions` on flat rows in (B, T) order."""
    pol = agent.policy
    hidden = pol.encode_observations(flat)
    y, state = agent.recurrent(hidden.view(b, t, -1).transpose(0, 1), state)
    return (*pol.decode_actions(y.transpose(0, 1).reshape(b * t, -1), flat, action), state)


def test_one_step_and_a_window_equal_the_composition_written_out(rows):
    agent, obs, _ = rows
    assert isinstance(agent.recurrent, nn.LSTM)
    kept = obs.clone()
    action = torch.stack([torch.zeros(B * T, dtype=torch.int64)] * 12, 1)
    state = (torch.randn(2, B, H), torch.randn(2, B, H))
    with torch.no_grad():
        for o, b, t, a, st in ((obs[:B], B, 1, action[:B], None), (obs[:B], B, 1, action[:B], state),
                               (obs.view(B, T, -1), B, T, action, state),
                               (obs.view(B, T, -1), B, T, action.view(B, T, 12), None)):
            got = agent(o, st, action=a)
            want = composed(agent, o.reshape(b * t, -1), b, t, st, a.reshape(b * t, 12))
            assert tuple(got[1].shape) == (b * t,) and tuple(got[3].shape) == (b * t, 1)
            assert tuple(got[4][0].shape) == tuple(got[4][1].shape) == (2, b, H)
            for x, y in zip(got[1:4], want[1:4]):
                assert torch.equal(x, y)
            assert torch.equal(got[4][0], want[4][0]) and torch.equal(got[4][1], want[4][1])
    assert torch.equal(obs, kept)


def test_outputs_are_in_batch_then_time_order(rows):
    """Row b * T + t of a window's outputs is step t of sequence b: the window equals T single steps
    that carry the state, and differs from the same rows read as (T, B)."""
    agent, obs, _ = rows
    action = torch.zeros(B * T, 12, dtype=torch.int64)
    win = obs.view(B, T, -1)
    with torch.no_grad():
        _, logp, _, value, state = agent(win, action=action)
        st = None
        for t in range(T):
            _, lp_t, _, v_t, st = agent(win[:, t], st, action=action[:B])
            # (the two runs use different GEMM shapes: equal to rounding, where a wrong order is off by O(0.1))
            assert torch.allclose(lp_t, logp.view(B, T)[:, t], rtol=1e-4, atol=1e-4)
            assert torch.allclose(v_t, value.view(B, T, 1)[:, t], rtol=1e-4, atol=1e-5)
        assert torch.allclose(st[0], state[0], atol=1e-5) and torch.allclose(st[1], state[1], atol=1e-5)
        swapped = agent(win.transpose(0, 1).contiguous(), action=action)[3]
    assert float((swapped - value).abs().max()) > 1e-3


# ---------------------------------------------------------------- greedy, unfused
def first_argmax(logits, legal, dims):
    """numpy: per head the first index of the maximum of where(legal, logit, -1e9)."""
    off = np.cumsum([0] + list(dims))
    x = np.where(legal, logits, np.float32(-1e9))
    return np.stack([x[:, off[k]:off[k + 1]].argmax(1) for k in range(len(dims))], 1)


def test_greedy_is_the_first_argmax_of_the_masked_logits_and_draws_nothing(rows):
    agent, obs, legal = rows
    pol = agent.policy
    with torch.no_grad():
        hidden = pol.encode_observations(obs)
        out = [pol.action_decoder.layers[name](hidden) for name, _ in DECODER_LAYERS]
        logits = pol.logits(out, {k: out[k] for k in pol.pointer}, obs)
        want = first_argmax(logits.numpy(), legal, pol.dims)
        torch.manual_seed(1)
        a1, lp1, ent1, v1 = pol(obs, greedy=True)
        torch.manual_seed(2)  # no generator is consulted
        a2, lp2, _, _ = pol(obs, greedy=True)
        _, lp3, ent3, v3 = pol(obs, action=a1)
    assert a1.dtype == torch.int64 and np.array_equal(a1.numpy(), want)
    assert torch.equal(a1, a2) and torch.equal(lp1, lp2)
    assert torch.equal(lp1, lp3) and torch.equal(ent1, ent3) and torch.equal(v1, v3)  # = evaluating the selection
    assert (want[0] == 0).all()  # row 0: nothing legal anywhere
    off = np.cumsum([0] + pol.dims)
    assert all(want[3, k] == pol.dims[k] - 1 for k in range(12))  # row 3: only the last entry legal
    assert all(legal[r, off[k] + want[r, k]] for r in range(1, len(want)) for k in range(12)
               if legal[r, off[k]:off[k + 1]].any())
    assert pol.draws == 0
    with torch.no_grad():  # through the recurrent wrapper, one step
        a4 = agent(obs, greedy=True)[0]
        h4 = composed(agent, obs, len(obs), 1, None, a4)
        assert torch.equal(agent(obs, action=a4)[1], h4[1])
    assert agent.draws == 0


def test_greedy_with_given_actions_raises(rows):
    agent, obs, _ = rows
    action = torch.zeros(len(obs), 12, dtype=torch.int64)
    with torch.no_grad():
        for call in (lambda: agent(obs, action=action, greedy=True), lambda: agent.policy(obs, action, greedy=True),
                     lambda: agent.policy.masked(torch.zeros(len(obs), 1586), obs, action, greedy=True)):
            with pytest.raises(ValueError, match="greedy"):
                call()
    cuda_free = torch.zeros(2, 5)
    for fn, args in ((heads.masked_heads, (cuda_free, torch.ones(2, 5), [2, 3])),
                     (heads.pointer_heads, (None, [], [-1, -1], cuda_free, torch.ones(2, 5), [2, 3]))):
        with pytest.raises(ValueError, match="greedy"):
            fn(*args, action=torch.zeros(2, 2, dtype=torch.int32), greedy=True)
    from nmmo_amd import decoder

    with pytest.raises(ValueError, match="greedy"):
        decoder.decoder_heads(cuda_free, None, [], [-1, -1], torch.ones(2, 5), [2, 3],
                              action=torch.zeros(2, 2, dtype=torch.int32), greedy=True)
    with pytest.raises(heads.HeadsError):  # no torch fallback for the fused selection either
        heads.masked_heads(cuda_free, torch.ones(2, 5), [2, 3], greedy=True)


# ---------------------------------------------------------------- the three new symbols
NEW = ["nmh_forward_argmax", "nmh_pointer_forward_argmax", "nmh_decoder_forward_argmax"]


def test_new_symbols_are_declared_in_header_symbols_and_ctypes():
    text = open(HEADER).read()
    L = heads.lib()
    for name, base in zip(NEW, ("nmh_forward", "nmh_pointer_forward", "nmh_decoder_forward")):
        assert re.search(rf"NMH_API int {name}\(", text), name
        assert name in heads.SYMBOLS
        got, full = getattr(L, name).argtypes, getattr(L, base).argtypes
        assert got is not None and len(got) == len(full) - 4
        # the base function's arguments without actions_in, seed, offset, row_base (the four before the outputs)
        assert list(got) == list(full[:-10]) + list(full[-6:]), name


def _dense(hd, n_rows=4, logits=0x1000, ls=None, mask=0x1000, ms=None, kind=0, outs=(0x1000,) * 5):
    total = sum(hd.dims[:max(0, min(hd.n_heads, 16))]) if hd is not None else 0
    return heads.lib().nmh_forward_argmax(
        None if hd is None else ctypes.byref(hd), n_rows, logits, total if ls is None else ls, mask,
        total if ms is None else ms, kind, *outs, None)


def test_forward_argmax_reports_argument_errors_without_a_gpu():
    """Every pointer is a non-null dummy that is never dereferenced: each call fails its check before
    any launch, with the base function's message under the new name."""
    L, E = heads.lib(), heads.NMH_E_INVALID
    good = heads.heads_struct(NMMO_DIMS)

    def bad(n_heads=12, **dims):
        hd = heads.heads_struct(NMMO_DIMS)
        hd.n_heads = n_heads
        for k, v in dims.items():
            hd.dims[int(k[1:])] = v
        return hd

    for what, kw in [("hd is NULL", dict(hd=None)), ("n_heads", dict(hd=bad(0))), ("n_heads", dict(hd=bad(17))),
                     ("dims[2]", dict(hd=bad(d2=0))), ("dims[2]", dict(hd=bad(d2=2049))),
                     ("NULL", dict(hd=good, logits=None)), ("NULL", dict(hd=good, mask=None)),
                     ("mask_kind", dict(hd=good, kind=2)), ("logits_stride", dict(hd=good, ls=1585)),
                     ("mask_stride", dict(hd=good, ms=1585)), ("n_rows", dict(hd=good, n_rows=-1))]:
        assert _dense(**kw) == E, what
        msg = L.nmh_last_error()
        assert msg.startswith(b"nmh_forward_argmax:") and what.encode() in msg, (what, msg)
    for i in range(5):
        outs = [0x1000] * 5
        outs[i] = None
        assert _dense(good, outs=tuple(outs)) == E and b"output pointer is NULL" in L.nmh_last_error()
    assert _dense(heads.heads_struct([2048] * 16), n_rows=0) == heads.NMH_OK  # zero rows: nothing is launched


class PointerArgs(test_pointer_heads_abi.Args):
    def argmax(self):
        return heads.lib().nmh_pointer_forward_argmax(
            self.hd_p, self.pt_p, self.n_rows, self.queries, self.array(self.keys), self.dense, self.dense_stride,
            self.mask, self.mask_stride, self.mask_kind, *self.out, None)


class DecoderArgs(test_decoder_abi.Args):
    def argmax(self):
        hd, st = self.structs()
        return heads.lib().nmh_decoder_forward_argmax(hd, st, self.n, self.pq, self.dense, self.dense_stride,
                                                      self.mask, self.mask_stride, self.mask_kind, self.a_out,
                                                      self.logprob, self.entropy, self.lse, self.hent, None)


def refused(a, name, *words):
    rc = a.argmax()
    msg = heads.lib().nmh_last_error().decode()
    assert rc == heads.NMH_E_INVALID, (rc, msg)
    assert msg.startswith(name + ":"), msg
    for w in words:
        assert str(w) in msg, (w, msg)


def test_pointer_forward_argmax_shares_the_base_functions_checks():
    name = "nmh_pointer_forward_argmax"
    assert PointerArgs().argmax() == heads.NMH_OK  # n_rows = 0
    for bend, words in ((dict(mask_kind=2), ("mask_kind", 2)), (dict(n_rows=-1), ("n_rows", -1)),
                        (dict(mask=None), ("mask is NULL",)), (dict(queries=0x1008), ("queries", "16-byte")),
                        (dict(hd_p=None), ("hd is NULL",)), (dict(pt_p=None), ("pt is NULL",)),
                        (dict(mask_stride=sum(NMMO_DIMS) - 1), ("mask_stride",)), (dict(dense=None), ("dense",))):
        a = PointerArgs()
        for k, v in bend.items():
            setattr(a, k, v)
        refused(a, name, *words)
    a = PointerArgs()
    a.pt.key_dim = 6
    refused(a, name, "key_dim", 6)
    a = PointerArgs(dims=[1025, 1025], head_set=[0, 0], set_rows=[1024], key_dim=64)
    refused(a, name, "sum(dims)", 2050)
    for i in range(5):
        a = PointerArgs()
        a.out[i] = None
        refused(a, name, "output", "NULL")


def test_decoder_forward_argmax_shares_the_base_functions_checks():
    name = "nmh_decoder_forward_argmax"
    assert DecoderArgs().argmax() == heads.NMH_OK  # n_rows = 0
    for bend, words in ((dict(hd=False), ("hd", "NULL")), (dict(st=False), ("sets", "NULL")),
                        (dict(elem=2), ("elem_kind", 2)), (dict(mask_kind=-1), ("mask_kind", -1)),
                        (dict(n=-1), ("n_rows", -1)),
                        (dict(rows=[257, 8], dims=[3, 258, 9, 9, 7]), ("set_rows[0]", 257)),
                        (dict(shares=[1, 0]), ("share[1]", 0)), (dict(mask_stride=33), ("mask_stride", 33, 34)),
                        (dict(dense_stride=9), ("dense_stride", 9, 10)), (dict(pq=None), ("pq", "NULL")),
                        (dict(pq=0x1004), ("pq", "16-byte")), (dict(head_set=[-1, 0, 0, 0, -1], dims=[3, 6, 6, 6, 7]),
                                                               ("no head uses set 1",))):
        a = DecoderArgs()
        for k, v in bend.items():
            setattr(a, k, v)
        refused(a, name, *words)
    for field in ("a_out", "logprob", "entropy", "lse", "hent"):
        a = DecoderArgs()
        setattr(a, field, None)
        refused(a, name, "output", "NULL")
