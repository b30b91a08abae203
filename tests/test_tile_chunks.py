"""The row partition of the tile encoder's backward (nmmo_amd/tile.py `n_chunks_for`, SPEC.md §19,
include/nmmo_heads.h nmh_tile_backward), on the CPU for every N in 0..4,200.

`tile_conv1` passes c = n_chunks_for(N) = min(64, ceil(N / 16)) chunks (at least 1); the entry point
derives R = ceil(N / c) rows per chunk and chunk k owns rows [k R, min(N, (k + 1) R)). Up to N = 1,024
a chunk holds at most 16 rows; from 1,025 on the cap makes R grow and the last chunks can be empty,
because c R may exceed N by up to c - 1 rows. tests/test_gpu_tile_backward_shapes.py runs the kernel
on the three N whose geometry is pinned at the end of this module.
"""

import pytest

from nmmo_amd import tile

N_MAX = 4200
CAP_CASES = {
    # N: (chunks, rows per chunk, rows of the last chunk that holds any, empty chunks)
    1024: (64, 16, 16, 0),
    1025: (64, 17, 5, 3),
    1088: (64, 17, 17, 0),
}


def rows_per_chunk(n, c):
    """R as nmh_tile_backward derives it from (n_rows, n_chunks)."""
    return -(-n // c)


def chunk_rows(n, c, k):
    """[lo, hi) of chunk k the way the kernel forms it: lo = k R, hi = min(lo + R, N); the chunk is
    empty when lo >= hi."""
    R = rows_per_chunk(n, c)
    lo = k * R
    return lo, min(lo + R, n)


def empty_chunks(n, c):
    """Closed form: the chunks behind the last row. ceil(N / R) chunks hold rows."""
    R = rows_per_chunk(n, c)
    return c if n == 0 else c - -(-n // R)


def test_constants_are_the_headers():
    assert (tile.MAX_CHUNKS, tile.CHUNK_ROWS) == (64, 16)


@pytest.mark.parametrize("lo", range(0, N_MAX + 1, 600))
def test_partition_for_every_row_count(lo):
    for n in range(lo, min(lo + 600, N_MAX + 1)):
        c = tile.n_chunks_for(n)
        assert c == max(1, min(64, -(-n // 16))), n
        R = rows_per_chunk(n, c)
        assert 1 <= c <= 64 and c * R >= n, n
        assert R <= 16 or c == 64, n  # more than 16 rows per chunk only at the cap
        assert (R > 16) == (n > 1024), n
        nxt, empty = 0, 0
        for k in range(c):
            a, b = chunk_rows(n, c, k)
            if a >= b:
                empty += 1
                assert a >= n, (n, k)  # nothing left for it
                continue
            assert a == nxt and b - a <= R and empty == 0, (n, k)  # contiguous, and no gap before rows
            assert b - a == R or b == n, (n, k)  # only the last chunk with rows is partial
            nxt = b
        assert nxt == n, n
        assert empty == empty_chunks(n, c), n
        assert empty < c or n == 0, n
        assert empty * R < n + R or n == 0, n


def test_empty_chunks_appear_only_above_the_cap():
    first = next(n for n in range(1, N_MAX + 1) if empty_chunks(n, tile.n_chunks_for(n)))
    assert first == 1025
    # below the cap, R = 16 would leave none; ceil(N / c) can still be smaller than 16
    assert all(empty_chunks(n, tile.n_chunks_for(n)) == 0 for n in range(1, 1025))
    assert max(empty_chunks(n, tile.n_chunks_for(n)) for n in range(1025, N_MAX + 1)) == 3


@pytest.mark.parametrize("n", sorted(CAP_CASES))
def test_the_gpu_modules_three_row_counts(n):
    c, R, last, empty = CAP_CASES[n]
    assert tile.n_chunks_for(n) == c and rows_per_chunk(n, c) == R and empty_chunks(n, c) == empty
    k_last = c - empty - 1
    a, b = chunk_rows(n, c, k_last)
    assert b == n and b - a == last
    for k in range(k_last + 1, c):
        a, b = chunk_rows(n, c, k)
        assert a >= b
    if n == 1025:
        assert k_last == 60 and chunk_rows(n, c, 60) == (1020, 1025)
