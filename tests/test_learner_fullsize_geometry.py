"""The geometry of tests/test_gpu_learner_fullsize.py, checked without a GPU: every strided view fits its
buffer, its stride is odd, and the row it names does hold the boundary inside the section of interest;
so a kernel that formed the row's offset in 32 bits would read another address."""

import pytest

from nmmo_amd import layout
from tests import test_gpu_learner_fullsize as fs

INT32_MAX = 2 ** 31 - 1


def test_the_buffer_is_the_c4_flat_obs():
    assert fs.W == layout.obs_elems(2048) == 23987 and fs.ROWS == 1024 * 128
    assert fs.BIG == 3_144_024_064 > fs.E31 and fs.BIG * 4 > fs.B32
    assert fs.TOTAL == 1586 and fs.section("mask") == (0, 1586)
    ends = [sum(fs.section(s)) for s in ("Entity", "Inventory", "Market", "Tile")]
    assert ends == [fs.I_OFF, fs.M_OFF, layout.flat_layout(2048)["Task"].offset, fs.W]
    assert fs.HEAD_OFF["Attack.Target"] == 3 and fs.HEAD_OFF["Buy.MarketItem"] == 104
    assert sum(fs.PDIMS) == fs.HEAD_OFF["Buy.MarketItem"]  # the pointer case's heads are the row's first two


@pytest.mark.parametrize("key", sorted(fs.GEO), ids=lambda k: f"{k[0]}-{k[1]}")
def test_a_view_straddles_its_boundary_inside_its_buffer(key):
    name, kind = key
    g = fs.GEO[key]
    off, length = fs.section(name)
    capacity = {"e31": fs.BIG, "b32": fs.BIG, "i16": fs.I16_ELEMS, "u8": fs.U8_ELEMS}[kind]
    assert g.itemsize == {"e31": 4, "b32": 4, "i16": 2, "u8": 1}[kind]
    assert g.n <= 9 and g.stride % 2 == 1 and g.stride >= g.width
    assert g.need == (g.n - 1) * g.stride + g.width <= capacity
    if kind in ("i16", "u8"):
        assert capacity - fs.E31 <= fs.W, "a buffer just past 2^31 elements"
        assert g.row == g.n - 1 and g.row * g.stride <= INT32_MAX  # (only the column offset crosses here)
    # the boundary, as an element offset from the view's (= the buffer's) first element
    want = fs.B32 // g.itemsize if kind == "b32" else fs.E31
    assert g.target == want and (kind != "i16" or g.target * g.itemsize == fs.B32)
    start = g.row * g.stride + off
    assert start < g.target < start + length - 1 and g.target - start == g.inside
    # the elements on both sides of it are the section's: the row's 32-bit offset would not reach them
    assert start + length - 1 > INT32_MAX if g.target == fs.E31 else (start + length - 1) * g.itemsize > 2 ** 32 - 1
    # no other row's section touches a boundary, and the rows after it lie wholly past it
    for r in range(g.n):
        if r != g.row:
            lo = r * g.stride + off
            assert not lo <= g.target < lo + length
            assert (lo > g.target) == (r > g.row)
    if kind == "e31":
        assert g.n - 1 - g.row >= 2 and (g.row + 1) * g.stride > INT32_MAX  # r * stride itself overflows int32
    if kind == "b32":
        assert sum(r * g.stride > INT32_MAX for r in range(g.n)) >= 2
    # rows at every alignment the element size allows modulo 16 bytes
    assert len({r * g.stride * g.itemsize % 16 for r in range(g.n)}) == min(16 // g.itemsize, g.n)


def test_every_entry_point_has_its_cases():
    for name in fs.F32_SECTIONS:
        assert (name, "e31") in fs.GEO and (name, "b32") in fs.GEO
    for name in ("Tile", "Entity", "Inventory", "Market"):
        assert (name, "i16") in fs.GEO
    assert ("mask", "u8") in fs.GEO and ("ptr", "u8") in fs.GEO
    # the pointer-heads case reads the row's first two heads alone: its views straddle inside those
    assert fs.section("ptr") == (0, sum(fs.PDIMS)) == (0, 104)
    for kind in ("e31", "b32", "u8"):
        assert 0 < fs.GEO["ptr", kind].inside < sum(fs.PDIMS) - 1


def test_the_gather_and_store_rows_surround_both_boundaries():
    w = fs.W
    assert fs.ROW_B32 * w * 4 < fs.B32 < (fs.ROW_B32 + 1) * w * 4
    assert fs.ROW_E31 * w < fs.E31 < (fs.ROW_E31 + 1) * w
    for row in (fs.ROW_B32, fs.ROW_E31):
        assert {row - 1, row, row + 1} <= set(fs.GATHER_ROWS)
    assert fs.GATHER_ROWS[0] == 0 and fs.GATHER_ROWS[-1] == fs.ROWS - 1 and len(fs.GATHER_ROWS) <= len(fs.SEL)
    assert fs.ROW_E31 + 3 < fs.STORE_CAPACITY  # the store's seven slots end three past the boundary row


def test_the_tiling_meets_every_wave_and_the_pattern_rows_are_in_range():
    assert fs.K == 37 and all(fs.K % p for p in range(2, 7))
    assert {(r % fs.K, r % 4) for r in range(fs.ROWS)} == {(p, w) for p in range(fs.K) for w in range(4)}
    assert len(set(fs.SEL)) == len(fs.SEL) == fs.N_A and max(fs.SEL) < fs.K
