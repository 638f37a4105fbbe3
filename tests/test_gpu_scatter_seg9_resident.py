"""GPU parity tests for pass 2 of the MSB flow (k_scatter_seg9) in its
two-blocks-per-CU form: keys, ranks and positions in registers, one u16
array for the per-wave counts and then the tile positions, keys and then
values reordered through one LDS buffer, the bucket of a tile counted from
abase in global memory, and the two small arrays that remain overlaid on
dead parts of the buffer and of the count array.

The key patterns shape ONE pass-2 tile (all keys of the pattern share the
top byte 0x5A, and pass 1 is stable, so the tile sees them in input order):
a tail tile of one key, of 8191 and of 8192; all 512 digits with equal
counts, interleaved and in runs; only digits 0 and 511, the ends of every
512-entry array; one digit filling the whole sub-tile of wave 0 or of wave
15 with the digits next to it empty. One more pattern spreads about 40 keys
over each of 256 (or 129, every other one and both ends) top bytes, so that
most tiles are nearly empty and the bucket search sees bucket 0, bucket 255
and empty buckets between populated ones.

The MSB flow is taken from 2^14 elements on, so a pattern shorter than that
runs twice: as it is, and followed by filler keys of another top byte that
bring it to 2^14 (then the pattern's bucket reaches k_scatter_seg9). The
low 47 bits are random, or zero so that the keys of a digit are equal and
only a stable pass keeps their values in order. The values of the pair sort
are a random permutation, so a key paired with the wrong value by the second
reorder round shows. Every output sits between canaries, workspaces start
out as 0xFF. Exact equality against a stable host sort."""
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
MSB_MIN = 1 << 14
TOP = 0x5A          # top byte of the patterns
FILL_TOP = 0xC3     # top byte of the filler

PATTERNS = [
    "tail_1",               # n = 2 * 8192 + 1: the third tile has one key
    "tail_8191",
    "tail_8192",
    "digits_interleaved",   # digit9 = i % 512: each wave, each digit once
                            # per group of 64
    "digits_runs16",        # digit9 = i // 16: 32 runs per wave sub-tile
    "ends_8191x0_1x511",
    "ends_1x0_8191x511",
    "wave0_full_digit200",
    "wave15_full_digit311",
    "wave0_full_digit511",
    "wave15_full_digit0",
    "top256_x40",           # 256 top bytes, 40 keys each, n = 10240
    "top129_x80",           # top bytes 0, 2, .., 254 and 255
]
LOWS = ["random", "zero"]


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


def _full_wave(rng, wave, digit):
    """one tile: `digit` fills the sub-tile of `wave` (512 keys) and occurs
    nowhere else, digit - 1 and digit + 1 do not occur at all"""
    free = np.array([d for d in range(512)
                     if abs(d - digit) > 1], dtype=np.uint64)
    dig = free[rng.integers(0, len(free), TILE)]
    dig[wave * 512:(wave + 1) * 512] = digit
    return dig


def _digits(pattern, rng):
    """(top bytes, 9-bit digits) of the pattern, in input order"""
    u = np.uint64
    if pattern.startswith("tail_"):
        tn = int(pattern[5:])
        n = 2 * TILE + tn if tn == 1 else tn
        return np.full(n, TOP, u), rng.integers(0, 512, n).astype(u)
    if pattern == "digits_interleaved":
        return np.full(TILE, TOP, u), (np.arange(TILE) % 512).astype(u)
    if pattern == "digits_runs16":
        return np.full(TILE, TOP, u), (np.arange(TILE) // 16).astype(u)
    if pattern.startswith("ends_"):
        many, one = (0, 511) if pattern == "ends_8191x0_1x511" else (511, 0)
        dig = np.full(TILE, many, u)
        dig[4001] = one
        return np.full(TILE, TOP, u), dig
    if pattern.startswith("wave"):
        wave, digit = pattern[4:].split("_full_digit")
        return (np.full(TILE, TOP, u),
                _full_wave(rng, int(wave), int(digit)).astype(u))
    if pattern == "top256_x40":
        tops = np.repeat(np.arange(256), 40)
    else:
        assert pattern == "top129_x80"
        tops = np.repeat(np.r_[np.arange(0, 256, 2), 255], 80)   # 10320
    tops = rng.permutation(tops).astype(u)
    return tops, rng.integers(0, 512, len(tops)).astype(u)


@functools.lru_cache(maxsize=None)
def make_keys(pattern, low, fill):
    rng = np.random.default_rng([PATTERNS.index(pattern),
                                 LOWS.index(low), int(fill)])
    u = np.uint64
    tops, dig = _digits(pattern, rng)
    n = len(tops)
    lo = (rng.integers(0, 1 << 47, n, dtype=np.uint64) if low == "random"
          else np.zeros(n, u))
    k = (tops << u(56)) | (dig << u(47)) | lo
    assert np.array_equal((k >> u(47)) & u(511), dig)
    if fill and n < MSB_MIN:
        f = rng.integers(0, 1 << 56, MSB_MIN - n, dtype=np.uint64)
        k = np.concatenate([k, (u(FILL_TOP) << u(56)) | f])
    return _frozen(k.astype(np.uint64))


def _cases():
    """every pattern with both kinds of low bits at a size that takes the
    MSB flow; a pattern shorter than that also as it is"""
    out = []
    for p in PATTERNS:
        short = p != "tail_1"
        combos = [(low, short) for low in LOWS]
        if short:
            combos.append(("random", False))
        for low, fill in combos:
            out.append(pytest.param(
                p, low, fill,
                id=f"{p}-{low}-{'filled' if fill else 'bare'}"))
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def pair_case(pattern, low, fill):
    """keys, values (a random permutation) and the stable host order"""
    keys = make_keys(pattern, low, fill)
    n = len(keys)
    vals = np.random.default_rng(n).permutation(n).astype(np.uint32)
    order = np.argsort(keys, kind="stable")
    return keys, _frozen(vals), _frozen(order)


@functools.lru_cache(maxsize=None)
def record_case(pattern, low, fill):
    """100-byte records whose big-endian 8-byte prefix is the pattern's
    key, and the same records in full-record byte order"""
    keys = make_keys(pattern, low, fill)
    n = len(keys)
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


@pytest.mark.parametrize("pattern,low,fill", CASES)
def test_pairs_permuted_values(nat, pattern, low, fill):
    keys, vals, order = pair_case(pattern, low, fill)
    n = len(keys)
    dk, dv = guarded(keys, np.uint64), guarded(vals, np.uint32)
    w = GD.filled_ws(nat.ws("sort_pairs", n))
    nat.sort_pairs_u64_u32(dk.ptr, dv.ptr, n, G.ptr(w), G.stream())
    GD.sync()
    assert np.array_equal(dk.read(), keys[order])
    assert np.array_equal(dv.read(), vals[order])


@pytest.mark.parametrize("pattern,low,fill", CASES)
def test_keys_only(nat, pattern, low, fill):
    keys, _, order = pair_case(pattern, low, fill)
    n = len(keys)
    dk = guarded(keys, np.uint64)
    w = GD.filled_ws(nat.ws("sort_u64", n))
    nat.sort_u64(dk.ptr, n, G.ptr(w), G.stream())
    GD.sync()
    assert np.array_equal(dk.read(), keys[order])


@pytest.mark.parametrize("pattern,low,fill", CASES)
def test_records(nat, pattern, low, fill):
    recs, expect = record_case(pattern, low, fill)
    n = len(recs)
    din = GD.In(recs.reshape(-1))
    dout = GD.Out(n * 100, np.uint8)
    w = GD.filled_ws(nat.ws("sort_records", n, 100))
    nat.sort_records(din.ptr, dout.ptr, n, 100, 10, G.ptr(w), G.stream())
    GD.sync()
    assert np.array_equal(dout.read().reshape(n, 100), expect)
    din.check()
