"""libnmmo_heads.so has one error text (nmmo_amd/csrc/heads_host.h, heads_fail): after a refused call
into any of its five translation units, nmh_last_error() holds that call's message, not the one a
call into another translation unit left before it. Every call passes n_rows = 0 and one bent
argument, as the ABI tests do, so nothing is launched. CPU only."""

import ctypes

import pytest

from nmmo_amd import heads, item

DUMMY = 0x1000  # non-null, 16-byte aligned, never dereferenced


def _hd(dims):
    hd = heads.NmhHeads()
    hd.n_heads = len(dims)
    for k, d in enumerate(dims):
        hd.dims[k] = d
    return hd


def _heads_hip(L):  # nmh_forward: hd is NULL
    return L.nmh_forward(None, 0, DUMMY, 8, DUMMY, 8, heads.MASK_F32, None, 1, 2, 3, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY,
                         None)


def _heads_hip_plan(L):  # nmh_pointer_forward, through the shared head plan: key set 0 has no head
    hd, pt = _hd([3]), heads.NmhPointer()
    pt.n_sets, pt.key_dim, pt.set_rows[0], pt.head_set[0] = 1, 8, 5, -1
    return L.nmh_pointer_forward(ctypes.byref(hd), ctypes.byref(pt), 0, DUMMY, (ctypes.c_void_p * 1)(DUMMY), DUMMY, 3,
                                 DUMMY, 3, heads.MASK_F32, None, 1, 2, 3, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, None)


def _tile_enc_hip(L):  # nmh_tile_forward: tile is NULL
    return L.nmh_tile_forward(0, None, 675, 0, DUMMY, DUMMY, DUMMY, None, None)


def _item_enc_hip(L):  # nmh_item_features: items is NULL
    return L.nmh_item_features(0, None, 16 * 4, 0, 4, DUMMY, DUMMY, None)


def _item_enc_hip_logits(L):  # nmh_item_logits, through the shared set rules: set_rows 0
    ih = item.item_heads_struct([0], [0])
    return L.nmh_item_logits(ctypes.byref(ih), 0, DUMMY, 64, 0, 0, 1, DUMMY, 8, heads.MASK_F32, DUMMY, DUMMY, 8, None)


def _player_enc_hip(L):  # nmh_player_features: ents is NULL
    return L.nmh_player_features(0, None, 31 * 4, 0, 4, None, 1, 0, DUMMY, DUMMY, None, None, None)


def _player_enc_hip_logits(L):  # nmh_player_logits, through the shared set rules: ph is NULL
    return L.nmh_player_logits(None, 0, DUMMY, 31 * 4, 0, 4, DUMMY, 8, heads.MASK_F32, DUMMY, DUMMY, 8, None)


def _decoder_hip(L):  # nmh_decoder_forward: sets is NULL
    hd = _hd([3])
    return L.nmh_decoder_forward(ctypes.byref(hd), None, 0, None, DUMMY, 3, DUMMY, 3, heads.MASK_F32, None, 1, 2, 3,
                                 DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, None)


CALLS = [
    (_heads_hip, "nmh_forward: hd is NULL"),
    (_tile_enc_hip, "nmh_tile_forward: tile is NULL"),
    (_item_enc_hip, "nmh_item_features: items is NULL"),
    (_player_enc_hip, "nmh_player_features: ents is NULL"),
    (_decoder_hip, "nmh_decoder_forward: sets is NULL"),
    (_heads_hip_plan, "nmh_pointer_forward: no head uses key set 0 (head_set)"),
    (_item_enc_hip_logits, "nmh_item_logits: set_rows 0 outside 1..1024"),
    (_player_enc_hip_logits, "nmh_player_logits: ph is NULL"),
]


@pytest.mark.parametrize("order", [1, -1], ids=["in_order", "reversed"])
def test_the_last_error_is_the_last_refused_calls_whatever_file_refused_it(order):
    L = heads.lib()
    for call, message in CALLS[::order]:
        assert call(L) == heads.NMH_E_INVALID, message
        assert L.nmh_last_error().decode() == message
