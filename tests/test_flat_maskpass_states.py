"""CPU: one no-op step on the oracle from each of tests/flat_maskpass_states.py's states leaves what
tests/test_gpu_flat_maskpass.py relies on, in agents 16 g + w + 4 j that share a wave of the flat obs
kernel: visible-row counts one below, at and one above the mask pass's lane group beside 1 and beside
more than 100, a same-tile attackable player at the last covered and the first uncovered row, the
listing counts with own and unaffordable listings at the edges of Buy's 64-listing words, inventories
of 0, 11 and 12 items with equipped and listed items at slots 0 and 11, the gold edges, a dangerous
NPC in attack range, and mixed waves."""

import numpy as np

from nmmo_amd import abi
from oracle.oracle import split_state
from tests import flat_maskpass_states as ms
from tests import obs_scenarios as sc

F = abi.F
K = ms.K_ROWS


def _orc():
    return sc.make_oracle(sc.config())


def test_lane_group_counts_share_a_wave():
    orc = _orc()
    (_, blob), = ms.group_states()
    c, post = ms.post_counts(orc, blob, ms.noop_actions())
    nv0, nv1 = c[0]["in_window"], c[1]["in_window"]
    print(nv0[[0, 4, 8, 12]], nv1[[0, 4, 8, 12]])
    assert {ms.wave_of(p) for p in (0, 4, 8, 12)} == {(0, 0)}
    assert nv0[[0, 4, 8, 12]].tolist() == [K - 1, K, K + 1, 1]
    # the last two members see what their observer sees, in other waves (beside agents that see fewer)
    for obs, mem in ms.CLUSTERS:
        assert all(nv0[m] == len(mem) for m in mem)
    for obs, mem in ms.CLUSTERS:  # the same-tile, attackable players are the cluster's last two rows
        n = len(mem)
        assert ms.same_tile_attackable(post, 0, obs, n - 2) and ms.same_tile_attackable(post, 0, obs, n - 1), obs
    assert ms.same_tile_attackable(post, 0, 8, K - 1) and ms.same_tile_attackable(post, 0, 8, K)  # rows 15 and 16
    assert ms.same_tile_attackable(post, 0, 4, K - 1)                                            # row 15 of 16
    assert nv1[0] == ms.BIG and nv1[[4, 8, 12]].tolist() == [1, 1, 1]
    assert c[1]["nv"][0] == 100
    inv = c[0]["ninv"]
    assert {0, 11, 12} <= set(inv.tolist())
    gold = split_state(post, sc.N_ENVS, 384, 128)["ent"][0, F["gold"], :128]
    assert {int(gold[p]) for p in (16, 20, 24, 28)} == {0, 1, 98, 99} and gold[17] == 100


def test_listing_counts_and_edges():
    orc = _orc()
    seen = []
    for name, blob in ms.listing_states():
        c, post = ms.post_counts(orc, blob, ms.noop_actions())
        d = split_state(post, sc.N_ENVS, 384, 128)
        for e in range(sc.N_ENVS):
            m = c[e]["priced"]
            seen.append(m)
            if m == 0:
                continue
            _, own, price = sc.priced_rows(d, e, 128)
            bits = sc.buy_bits(d, e, 128)
            gold = d["ent"][e, F["gold"], :128].astype(np.int64)
            alive = d["ent"][e, F["alive"], :128] != 0
            for k in {0, min(m, 64) - 1, m - 1}:  # the edges of Buy's words 0 and (from 960 listings) 15
                o = int(own[k])
                assert alive[o] and gold[o] >= price[k] and bits[o, k] == 0, (name, e, k)  # its own listing
                assert ((gold < price[k]) & alive).any() and (bits[alive, k] == 1).any(), (name, e, k)
        # equipped and listed items at slots 0 and 11 of a full inventory, and inventories of 0 and 11
        it = d["items"][0].astype(np.int64)
        full = c[0]["ninv"] == 12
        eq, listed = (it[:, :, 0] >> 9) & 1, (it[:, :, 0] >> 10) & 127
        for k in (0, 11):
            assert (eq[full, k] != 0).any(), (name, k)
            if c[0]["priced"] >= 900:  # (a few listings over 128 inventories need not reach both slots)
                assert (listed[full, k] != 0).any(), (name, k)
        # (the largest counts top the inventories up)
        assert ({0, 11, 12} if c[0]["priced"] < 900 else {12}) <= set(c[0]["ninv"].tolist())
        nv = c[0]["in_window"][:ms.CROWD]
        print(name, nv.tolist())
        assert nv.max() > K and 0 < nv[nv > 0].min() <= K  # the crowd and its NPCs: both sides of the lane group
    print(seen)
    assert seen == list(ms.LISTING_COUNTS), seen


def test_dangerous_npc_in_attack_range():
    c, post = ms.post_counts(_orc(), ms.danger_state()[1], ms.noop_actions())
    ent = split_state(post, sc.N_ENVS, 384, 128)["ent"][0].astype(np.int64)
    npc = [s for s in range(128, 384) if ent[F["alive"], s] and ent[F["npc_type"], s] > 1]
    pl = np.flatnonzero(ent[F["alive"], :128])
    assert any((np.maximum(np.abs(ent[F["row"], pl] - ent[F["row"], s]), np.abs(ent[F["col"], pl] - ent[F["col"], s])) <= 3).any()
               for s in npc)


def test_mixed_waves():
    a, b = ms.mixed_states()
    orc = _orc()
    ca, _ = ms.post_counts(orc, a, ms.noop_actions())
    cb, _ = ms.post_counts(orc, b, ms.noop_actions())
    for e in range(sc.N_ENVS):
        out = cb[e]["nv"] < 0
        assert (ca[e]["nv"] >= 0).all() and out[list(sc.GROUP_OUT)].all() and out.sum() == len(sc.GROUP_OUT)
        waves = {}
        for p in range(128):
            waves.setdefault(ms.wave_of(p), []).append(bool(out[p]))
        assert any(all(v) for v in waves.values())                  # a whole wave out
        assert any(any(v) and not all(v) for v in waves.values())   # a wave with both kinds
