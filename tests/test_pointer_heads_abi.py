"""The pointer-head entry points of libnmmo_heads.so (include/nmmo_heads.h, SPEC.md §18) without a
GPU: the ctypes mirror matches the header as a C compiler lays it out, and every rule of §18's
"Limits" is refused with NMH_E_INVALID and a message naming the field. Every call passes dummy
non-null pointers and n_rows <= 0, so a check that is missing shows as NMH_OK, never as a launch.
CPU only."""

import ctypes
import os
import subprocess
import tempfile

import pytest

from nmmo_amd import heads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = 0x1000  # non-null, 16-byte aligned, never dereferenced
NMMO_DIMS = [3, 101, 1025, 13, 13, 101, 99, 101, 5, 13, 99, 13]
NMMO_SETS = [-1, 0, 2, 1, 1, 0, -1, 0, -1, 1, -1, 1]
NMMO_ROWS = [100, 12, 1024]


def test_constants_and_struct_match_the_c_compiler():
    src = r"""
#include <stdio.h>
#include <stddef.h>
#include "nmmo_heads.h"
int main(void) {
  printf("%d %d %d %d %zu %zu %zu %zu %zu %zu\n", NMH_MAX_HEADS, NMH_MAX_DIM, NMH_MAX_SETS, NMH_MAX_KEY_DIM,
         sizeof(NmhPointer), offsetof(NmhPointer, n_sets), offsetof(NmhPointer, key_dim),
         offsetof(NmhPointer, set_rows), offsetof(NmhPointer, head_set), sizeof(NmhHeads));
  return 0;
}
"""
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        with open(c, "w") as fh:
            fh.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    P = heads.NmhPointer
    assert got == [heads.MAX_HEADS, heads.MAX_DIM, heads.MAX_SETS, heads.MAX_KEY_DIM, ctypes.sizeof(P),
                   P.n_sets.offset, P.key_dim.offset, P.set_rows.offset, P.head_set.offset,
                   ctypes.sizeof(heads.NmhHeads)]
    assert got[:4] == [16, 2048, 4, 256] and got[4] == 88


class Args:
    """Valid arguments for the 12 nmmo heads at D = 64 and n_rows = 0; a test bends one of them."""

    def __init__(self, dims=NMMO_DIMS, head_set=NMMO_SETS, set_rows=NMMO_ROWS, key_dim=64):
        self.hd = heads.NmhHeads()
        self.hd.n_heads = len(dims)
        for k, d in enumerate(dims):
            self.hd.dims[k] = d
        self.pt = heads.NmhPointer()
        self.pt.n_sets, self.pt.key_dim = len(set_rows), key_dim
        for s, m in enumerate(set_rows):
            self.pt.set_rows[s] = m
        for k, s in enumerate(head_set):
            self.pt.head_set[k] = s
        self.hd_p, self.pt_p = ctypes.byref(self.hd), ctypes.byref(self.pt)
        self.n_rows = 0
        self.queries = self.dense = self.mask = self.actions = self.g_dense = self.g_queries = DUMMY
        self.out = [DUMMY] * 5  # actions_out, logprob, entropy, lse, head_entropy
        self.saved = [DUMMY] * 3  # actions, lse, head_entropy
        self.keys = [DUMMY] * heads.MAX_SETS
        self.g_keys = [DUMMY] * heads.MAX_SETS
        self.dense_stride = self.g_dense_stride = sum(d for d, s in zip(dims, head_set) if s < 0)
        self.mask_stride = sum(dims)
        self.mask_kind = heads.MASK_F32

    @staticmethod
    def array(ptrs):
        return None if ptrs is None else (ctypes.c_void_p * len(ptrs))(*ptrs)

    def forward(self):
        return heads.lib().nmh_pointer_forward(
            self.hd_p, self.pt_p, self.n_rows, self.queries, self.array(self.keys), self.dense, self.dense_stride,
            self.mask, self.mask_stride, self.mask_kind, None, 1, 2, 3, *self.out, None)

    def backward(self):
        return heads.lib().nmh_pointer_backward(
            self.hd_p, self.pt_p, self.n_rows, self.queries, self.array(self.keys), self.dense, self.dense_stride,
            self.mask, self.mask_stride, self.mask_kind, *self.saved, DUMMY, DUMMY, self.g_dense,
            self.g_dense_stride, self.g_queries, self.array(self.g_keys), None)


def refused(a, *words, calls=("forward", "backward")):
    for fn in calls:
        rc = getattr(a, fn)()
        msg = heads.lib().nmh_last_error().decode()
        assert rc == heads.NMH_E_INVALID, (fn, rc, msg)
        assert msg.startswith(f"nmh_pointer_{fn}:"), msg
        for w in words:
            assert w in msg, (fn, w, msg)


def test_valid_arguments_with_no_rows_are_a_no_op():
    a = Args()
    assert a.forward() == heads.NMH_OK and a.backward() == heads.NMH_OK
    # NULL gradient outputs are "do not compute", not errors
    a.g_dense, a.g_queries, a.g_keys = None, None, None
    assert a.backward() == heads.NMH_OK
    a.g_keys = [None, DUMMY, None, None]
    assert a.backward() == heads.NMH_OK
    # all heads dense: no sets, queries and keys NULL, key_dim not looked at
    b = Args(dims=[3, 5], head_set=[-1, -1], set_rows=[], key_dim=0)
    b.queries, b.keys, b.g_keys = None, None, None
    assert b.forward() == heads.NMH_OK and b.backward() == heads.NMH_OK
    # all heads pointers: dense NULL
    c = Args(dims=[6, 6], head_set=[0, 0], set_rows=[5], key_dim=4)
    c.dense = c.g_dense = None
    assert c.forward() == heads.NMH_OK and c.backward() == heads.NMH_OK


def test_sum_of_dims_beyond_one_tile_is_refused():
    a = Args(dims=[1025, 1025], head_set=[0, 0], set_rows=[1024], key_dim=64)
    refused(a, "sum(dims)", "2050")
    assert Args(dims=[1024, 1024], head_set=[0, 0], set_rows=[1023], key_dim=64).forward() == heads.NMH_OK


def test_too_many_sets_are_refused():
    a = Args()
    a.pt.n_sets = heads.MAX_SETS + 1
    refused(a, "n_sets", "5")
    a.pt.n_sets = -1
    refused(a, "n_sets", "-1")


def test_an_unused_set_is_refused():
    a = Args()
    a.pt.n_sets = 4
    a.pt.set_rows[3] = 7
    refused(a, "key set 3", "head_set")


@pytest.mark.parametrize("key_dim", [0, 2, 6, 63, 260, -4])
def test_bad_key_dim_is_refused(key_dim):
    a = Args()
    a.pt.key_dim = key_dim
    refused(a, "key_dim", str(key_dim))


def test_head_size_must_be_set_rows_plus_one():
    a = Args()
    a.pt.set_rows[1] = 13
    refused(a, "dims[3]", "set_rows[1]")
    a = Args()
    a.pt.head_set[0] = 3
    refused(a, "head_set[0]", "3")
    a = Args()
    a.pt.set_rows[2] = 0
    refused(a, "set_rows[2]")


def test_bad_heads_are_refused():
    a = Args()
    a.hd.n_heads = 0
    refused(a, "n_heads")
    a = Args()
    a.hd.n_heads = heads.MAX_HEADS + 1
    refused(a, "n_heads")
    a = Args()
    a.hd.dims[0] = 0
    refused(a, "dims[0]")


def test_null_arguments_are_refused():
    for field, word in (("hd_p", "hd"), ("pt_p", "pt"), ("mask", "mask"), ("queries", "queries"),
                        ("keys", "keys"), ("dense", "dense")):
        a = Args()
        setattr(a, field, None)
        refused(a, word + " is NULL" if field in ("hd_p", "pt_p", "mask") else word)
    a = Args()
    a.keys[1] = None
    refused(a, "keys[1]", "NULL")
    for i in range(5):
        a = Args()
        a.out[i] = None
        refused(a, "output", calls=("forward",))
    for i in range(3):
        a = Args()
        a.saved[i] = None
        refused(a, "NULL", calls=("backward",))


def test_unaligned_pointers_are_refused():
    a = Args()
    a.keys[2] = DUMMY + 4
    refused(a, "keys[2]", "16-byte")
    a = Args()
    a.queries = DUMMY + 8
    refused(a, "queries", "16-byte")
    a = Args()
    a.g_keys[0] = DUMMY + 4
    refused(a, "g_keys[0]", "16-byte", calls=("backward",))
    a = Args()
    a.g_queries = DUMMY + 4
    refused(a, "g_queries", "16-byte", calls=("backward",))


def test_bad_mask_kind_rows_and_strides_are_refused():
    a = Args()
    a.mask_kind = 2
    refused(a, "mask_kind", "2")
    a = Args()
    a.n_rows = -1
    refused(a, "n_rows", "-1")
    a = Args()
    a.mask_stride = sum(NMMO_DIMS) - 1
    refused(a, "mask_stride")
    a = Args()
    a.dense_stride -= 1
    refused(a, "dense_stride")
    a = Args()
    a.g_dense_stride -= 1
    refused(a, "g_dense_stride", calls=("backward",))


def test_python_wrapper_rejects_wrong_layouts_before_any_call():
    with pytest.raises(ValueError, match="key width"):
        heads.pointer_struct([6], [0], [5], 6)
    with pytest.raises(ValueError, match="no-op"):
        heads.pointer_struct([7], [0], [5], 8)
    with pytest.raises(ValueError, match="no head uses"):
        heads.pointer_struct([6], [0], [5, 5], 8)
    with pytest.raises(ValueError, match="head_set"):
        heads.pointer_struct([6, 3], [0], [5], 8)
    with pytest.raises(ValueError, match="at most"):
        heads.pointer_struct([6], [0], [5] * 5, 8)
    pt = heads.pointer_struct(NMMO_DIMS, NMMO_SETS, NMMO_ROWS, 64)
    assert pt.n_sets == 3 and pt.key_dim == 64 and list(pt.set_rows)[:3] == NMMO_ROWS
    assert list(pt.head_set)[:12] == NMMO_SETS
