"""GPU parity tests for the two radix scatter passes of the MSB flow
(k_scatter_wave512 at the 8192 tile and k_scatter_seg9). Pass 1 keeps its
ranks and positions in registers, counts in one u16 array that is scanned
in place, and reorders the keys and then the values through one LDS
buffer; pass 2 counts in u16 rows as well.

The sizes give a ragged last pass-1 tile and bucket tails that are no
multiple of the tile in pass 2. The key patterns drive the u16 counters to
their largest count (a full wave sub-tile in one digit), offset and rank
(a full tile in one digit), in pass 1, in pass 2 or in both; the values of
the pair sort are a random permutation, so that a key paired with the wrong
value by the second reorder round shows. Every output sits between
canaries. Exact equality against a stable host sort."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tests import _gpu as G
    from tests import _guard as GD
    from thrill_amd import Native

TILE = 8192
SIZES = [1 << 14, (1 << 14) + 1, 3 * TILE - 1, 3 * TILE + 1]
PATTERNS = ["uniform", "all_equal", "one_top_byte", "one_top_byte_one_digit9",
            "two_top_bytes_alternating"]


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = Native(device=0)
    yield n
    n.close()


@pytest.fixture(autouse=True)
def msb_env():
    old = os.environ.get("T9_SORT_ALGO")
    os.environ["T9_SORT_ALGO"] = "msb"      # MSB flow from n = 2^14
    yield
    if old is None:
        del os.environ["T9_SORT_ALGO"]
    else:
        os.environ["T9_SORT_ALGO"] = old


def _frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def make_keys(pattern, n):
    rng = np.random.default_rng([PATTERNS.index(pattern), n])
    u = np.uint64
    rnd = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    if pattern == "uniform":
        k = rnd
    elif pattern == "all_equal":
        k = np.full(n, 0xABCDEF0123456789, dtype=np.uint64)
    elif pattern == "one_top_byte":
        # pass 1: the whole tile is one run; bits 47..55 stay uniform
        k = (u(0x5A) << u(56)) | (rnd >> u(8))
    elif pattern == "one_top_byte_one_digit9":
        # pass 2 as well: one 9-bit digit, only the low 47 bits vary
        k = (u(0x5A) << u(56)) | (u(0x1B3) << u(47)) | (rnd >> u(17))
    else:
        # neighbours differ in the top byte: two ballot groups of 32 lanes
        top = np.where(np.arange(n) % 2 == 0, u(0x11), u(0xEE)).astype(u)
        k = (top << u(56)) | (rnd >> u(8))
    return _frozen(k.astype(np.uint64))


@functools.lru_cache(maxsize=None)
def pair_case(pattern, n):
    """keys, values (a random permutation) and the stable host order"""
    keys = make_keys(pattern, n)
    vals = np.random.default_rng(n).permutation(n).astype(np.uint32)
    order = np.argsort(keys, kind="stable")
    return keys, _frozen(vals), _frozen(order)


@functools.lru_cache(maxsize=None)
def record_case(pattern, n):
    """100-byte records whose big-endian 8-byte prefix is the pattern's
    key, and the same records in full-record byte order"""
    keys = make_keys(pattern, n)
    recs = np.random.default_rng(n + 1).integers(
        0, 256, (n, 100)).astype(np.uint8)
    recs[:, :8] = keys.astype(">u8").view(np.uint8).reshape(n, 8)
    order = np.lexsort(tuple(recs[:, c] for c in range(99, -1, -1)))
    return _frozen(recs), _frozen(recs[order])


def guarded(arr, dtype):
    """an in-place device buffer holding arr between canaries"""
    o = GD.Out(len(arr), dtype)
    o.t[GD.NCAN:GD.NCAN + len(arr)].copy_(G.dev(np.array(arr)))
    return o


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_pairs_permuted_values(nat, pattern, n):
    keys, vals, order = pair_case(pattern, n)
    dk, dv = guarded(keys, np.uint64), guarded(vals, np.uint32)
    w = GD.filled_ws(nat.ws("sort_pairs", n))
    nat.sort_pairs_u64_u32(dk.ptr, dv.ptr, n, G.ptr(w), G.stream())
    GD.sync()
    assert np.array_equal(dk.read(), keys[order])
    assert np.array_equal(dv.read(), vals[order])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_keys_only(nat, pattern, n):
    keys, _, order = pair_case(pattern, n)
    dk = guarded(keys, np.uint64)
    w = GD.filled_ws(nat.ws("sort_u64", n))
    nat.sort_u64(dk.ptr, n, G.ptr(w), G.stream())
    GD.sync()
    assert np.array_equal(dk.read(), keys[order])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_records_iota_values(nat, pattern, n):
    recs, expect = record_case(pattern, n)
    din = GD.In(recs.reshape(-1))
    dout = GD.Out(n * 100, np.uint8)
    w = GD.filled_ws(nat.ws("sort_records", n, 100))
    nat.sort_records(din.ptr, dout.ptr, n, 100, 10, G.ptr(w), G.stream())
    GD.sync()
    assert np.array_equal(dout.read().reshape(n, 100), expect)
    din.check()
