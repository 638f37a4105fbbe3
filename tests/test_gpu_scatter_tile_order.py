"""GPU parity tests for the tile order and the clamped single key read of
the pass-1 radix scatter (k_scatter_wave512).

A block no longer works on tile blockIdx.x: block b takes tile
(b % 8) * (grid / 8) + b / 8, the remainder of grid / 8 going to the first
XCDs, so the tile base, the tile length and the row of the offset table all
follow the tile. The grids here are those at which that mapping can go
wrong: fewer tiles than XCDs (1, 7), exactly one or two per XCD (8, 16), a
remainder of one (9, 17) and of seven (15, 23). Every grid comes with a last
tile of 1, of 8191 and of 8192 keys: a lane past the end of a ragged tile
now loads a key at an index clamped into the tile, and such a key must take
no part in the match or in the counts.

The public pair sort carries a random permutation as values, so a key that
leaves with the wrong value shows; the keys-only sort and the 100-byte
record sort (the index-as-payload form behind the fused extract histogram)
run over the same keys. The pair sort runs once more under the LSD flow,
whose tiles share the kernel. Every output sits between canaries. Exact
equality against a stable host sort."""
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
GRIDS = [1, 7, 8, 9, 15, 16, 17, 23]
LAST = [1, TILE - 1, TILE]
SIZES = [(g - 1) * TILE + last for g in GRIDS for last in LAST]
assert max(SIZES) == 188416
PATTERNS = ["uniform", "one_top_byte", "two_top_bytes_alternating"]


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = Native(device=0)
    yield n
    n.close()


@pytest.fixture
def algo():
    """sets T9_SORT_ALGO for one test and restores it"""
    old = os.environ.get("T9_SORT_ALGO")

    def use(name):
        os.environ["T9_SORT_ALGO"] = name

    yield use
    if old is None:
        os.environ.pop("T9_SORT_ALGO", None)
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
    elif pattern == "one_top_byte":
        # the whole tile is one run of pass 1
        k = (u(0x5A) << u(56)) | (rnd >> u(8))
    else:
        # neighbouring lanes differ in the top byte: two match groups of 32
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
    key, and the same records in full-record byte order. The keys of these
    patterns are distinct (checked), so the key order is the record order."""
    keys, _, order = pair_case(pattern, n)
    assert len(np.unique(keys)) == n
    recs = np.random.default_rng(n + 1).integers(
        0, 256, (n, 100)).astype(np.uint8)
    recs[:, :8] = keys.astype(">u8").view(np.uint8).reshape(n, 8)
    return _frozen(recs), _frozen(recs[order])


def guarded(arr, dtype):
    """an in-place device buffer holding arr between canaries"""
    o = GD.Out(len(arr), dtype)
    o.t[GD.NCAN:GD.NCAN + len(arr)].copy_(G.dev(np.array(arr)))
    return o


def run_pairs(nat, pattern, n):
    keys, vals, order = pair_case(pattern, n)
    dk, dv = guarded(keys, np.uint64), guarded(vals, np.uint32)
    w = GD.filled_ws(nat.ws("sort_pairs", n))
    nat.sort_pairs_u64_u32(dk.ptr, dv.ptr, n, G.ptr(w), G.stream())
    GD.sync()
    assert np.array_equal(dk.read(), keys[order])
    assert np.array_equal(dv.read(), vals[order])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_pairs_permuted_values(nat, algo, pattern, n):
    algo("msb")
    run_pairs(nat, pattern, n)


@pytest.mark.parametrize("n", SIZES)
def test_pairs_lsd_tiles(nat, algo, n):
    algo("lsd")
    run_pairs(nat, "uniform", n)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_keys_only(nat, algo, pattern, n):
    algo("msb")
    keys, _, order = pair_case(pattern, n)
    dk = guarded(keys, np.uint64)
    w = GD.filled_ws(nat.ws("sort_u64", n))
    nat.sort_u64(dk.ptr, n, G.ptr(w), G.stream())
    GD.sync()
    assert np.array_equal(dk.read(), keys[order])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_records_iota_values(nat, algo, pattern, n):
    algo("msb")
    recs, expect = record_case(pattern, n)
    din = GD.In(recs.reshape(-1))
    dout = GD.Out(n * 100, np.uint8)
    w = GD.filled_ws(nat.ws("sort_records", n, 100))
    nat.sort_records(din.ptr, dout.ptr, n, 100, 10, G.ptr(w), G.stream())
    GD.sync()
    assert np.array_equal(dout.read().reshape(n, 100), expect)
    din.check()
