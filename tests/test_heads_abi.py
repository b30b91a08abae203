"""libnmmo_heads.so (include/nmmo_heads.h) loads without a GPU, its ctypes mirror matches the
header, and it reports argument errors through the return code + nmh_last_error without touching
a GPU. Its exports and source hash: tests/test_native_libs.py. CPU only."""

import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nmmo_heads.h")
NMMO_DIMS = [3, 101, 1025, 13, 13, 101, 99, 101, 5, 13, 99, 13]


@pytest.fixture(scope="module")
def heads():
    from nmmo_amd import heads

    heads.lib()
    return heads


def test_struct_and_constants_match_header(heads):
    text = open(HEADER).read()
    for macro, val in [("NMH_MAX_HEADS", heads.MAX_HEADS), ("NMH_MAX_DIM", heads.MAX_DIM),
                       ("NMH_MASK_F32", heads.MASK_F32), ("NMH_MASK_U8", heads.MASK_U8),
                       ("NMH_OK", heads.NMH_OK), ("NMH_E_INVALID", heads.NMH_E_INVALID),
                       ("NMH_E_HIP", heads.NMH_E_HIP)]:
        m = re.search(rf"#define {macro} (.*?)(?:/\*|$)", text, re.M)
        assert eval(m.group(1).strip()) == val, macro
    assert ctypes.sizeof(heads.NmhHeads) == 4 * (1 + heads.MAX_HEADS)


def _forward(heads, hd, n_rows=4, logits=0x1000, ls=None, mask=0x1000, ms=None, kind=0, outs=(0x1000,) * 5):
    total = sum(hd.dims[:max(0, min(hd.n_heads, 16))]) if hd is not None else 0
    return heads.lib().nmh_forward(
        None if hd is None else ctypes.byref(hd), n_rows, logits, total if ls is None else ls, mask,
        total if ms is None else ms, kind, None, 1, 0, 0, *outs, None)


def _backward(heads, hd, n_rows=4, logits=0x1000, ls=None, mask=0x1000, ms=None, kind=0, actions=0x1000, lse=0x1000,
              hent=0x1000, g=0x1000, gs=None):
    total = sum(hd.dims[:max(0, min(hd.n_heads, 16))]) if hd is not None else 0
    return heads.lib().nmh_backward(
        None if hd is None else ctypes.byref(hd), n_rows, logits, total if ls is None else ls, mask,
        total if ms is None else ms, kind, actions, lse, hent, None, None, g, total if gs is None else gs, None)


def test_argument_errors_are_reported_without_a_gpu(heads):
    """Every pointer below is a non-null dummy that is never dereferenced: each call must fail its
    argument check before any launch."""
    L, E = heads.lib(), heads.NMH_E_INVALID
    good = heads.heads_struct(NMMO_DIMS)

    def bad_heads(n_heads=12, **dims):
        hd = heads.heads_struct(NMMO_DIMS)
        hd.n_heads = n_heads
        for k, v in dims.items():
            hd.dims[int(k[1:])] = v
        return hd

    cases = [
        ("hd is NULL", dict(hd=None)),
        ("n_heads", dict(hd=bad_heads(0))),
        ("n_heads", dict(hd=bad_heads(17))),
        ("dims[2]", dict(hd=bad_heads(d2=0))),
        ("dims[2]", dict(hd=bad_heads(d2=2049))),
        ("dims[11]", dict(hd=bad_heads(d11=-3))),
        ("NULL", dict(hd=good, logits=None)),
        ("NULL", dict(hd=good, mask=None)),
        ("mask_kind", dict(hd=good, kind=2)),
        ("mask_kind", dict(hd=good, kind=-1)),
        ("logits_stride", dict(hd=good, ls=1585)),
        ("mask_stride", dict(hd=good, ms=1585)),
        ("n_rows", dict(hd=good, n_rows=-1)),
    ]
    for what, kw in cases:
        for fn in (_forward, _backward):
            assert fn(heads, **kw) == E, (fn.__name__, what)
            assert what.encode() in L.nmh_last_error(), (fn.__name__, what, L.nmh_last_error())
    for i in range(5):  # each forward output pointer
        outs = [0x1000] * 5
        outs[i] = None
        assert _forward(heads, good, outs=tuple(outs)) == E and b"NULL" in L.nmh_last_error()
    for kw in (dict(actions=None), dict(lse=None), dict(hent=None), dict(g=None)):
        assert _backward(heads, good, **kw) == E and b"NULL" in L.nmh_last_error()
    assert _backward(heads, good, gs=1585) == E and b"g_stride" in L.nmh_last_error()
    # the largest legal shapes pass the checks: zero rows is a no-op that launches nothing
    big = heads.heads_struct([2048] * 16)
    assert _forward(heads, big, n_rows=0) == heads.NMH_OK
    assert _backward(heads, big, n_rows=0) == heads.NMH_OK


def test_python_wrapper_rejects_bad_shapes_before_the_library(heads):
    import torch

    with pytest.raises(ValueError):
        heads.heads_struct([])
    with pytest.raises(ValueError):
        heads.heads_struct([2] * 17)
    with pytest.raises(heads.HeadsError):  # no torch fallback: host tensors are an error
        heads.masked_heads(torch.zeros(2, 5), torch.ones(2, 5), [2, 3])
