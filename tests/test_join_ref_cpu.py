"""The join tests' numpy checker (tests/_join_ref.py) against the definition
by a brute-force double loop, on shapes small enough for the loop: empty
sides, many keys, one key, almost no matches, each with one pair of keys at
2^64-1 (no value is a sentinel)."""
import numpy as np
import pytest

from tests import _join_ref as J

TOP = np.uint64(0xFFFFFFFFFFFFFFFF)

# (n_left, n_right, distinct keys)
SHAPES = [(0, 150, 40), (200, 0, 40), (200, 150, 40), (333, 50, 1),
          (300, 300, 10 ** 6)]


def sides(nl, nr, nkeys, top):
    rng = np.random.default_rng(nl * 1000 + nr)
    lk = rng.integers(0, nkeys, nl, dtype=np.uint64)
    rk = rng.integers(0, nkeys, nr, dtype=np.uint64)
    if top and nl and nr:
        lk[nl // 2] = TOP
        rk[nr // 3] = TOP
    return lk, rk


@pytest.mark.parametrize("top", [False, True], ids=["plain", "top-key"])
@pytest.mark.parametrize("nl,nr,nkeys", SHAPES)
def test_ref_matches_brute_force(nl, nr, nkeys, top):
    lk, rk = sides(nl, nr, nkeys, top)
    li, ri = J.join(lk, rk)
    bl, br = J.brute(lk, rk)
    assert li.dtype == np.uint32 and ri.dtype == np.uint32
    assert np.array_equal(li, bl)
    assert np.array_equal(ri, br)
    assert J.total(lk, rk) == len(bl)
    if top and nl and nr:
        # the pair at 2^64-1 sorts last
        assert lk[li[-1]] == TOP and rk[ri[-1]] == TOP


def test_ref_order_is_key_then_left_then_right():
    lk = np.array([5, 3, 5, 3], np.uint64)
    rk = np.array([3, 5, 5], np.uint64)
    li, ri = J.join(lk, rk)
    assert li.tolist() == [1, 3, 0, 0, 2, 2]
    assert ri.tolist() == [0, 0, 1, 2, 1, 2]
