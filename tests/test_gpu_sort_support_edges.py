"""Boundary-shape parity of the sort support kernels — group_index,
merge_u64, merge_records, classify_u64, classify_rec, partition_idx,
gather_records, extract_key64(_le) — against the numpy references of
tests/_np_ref.py. Every comparison is exact equality.

The size ladders are built from the kernel geometry in tests/_np_ref.py
(pinned to the sources by test_np_ref_cpu.py) and cross every tile, span,
chunk and grid-stride boundary at the smallest size that reaches it.
Outputs sit between canaries, workspaces start as 0xFF, counters that the
call must zero start as garbage, and inputs are checked for changes
(tests/_guard.py)."""
import numpy as np
import pytest
import torch

from tests import _np_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tests import _guard as U

ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
BIG = np.uint64(1 << 32)


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from thrill_amd import Native
    n = Native(device=0)
    yield n
    n.close()


@pytest.fixture(scope="module")
def stream():
    from tests import _gpu as G
    return G.stream()


def rand_u64(rng, n):
    return rng.integers(0, 1 << 64, n, dtype=np.uint64)


def be_prefix(recs, off=0):
    return recs[:, off:off + 8].copy().view(">u8").ravel().astype(np.uint64)


# ------------------------------------------------------------ group_index

GT = R.GRP_TILE
GROUP_SIZES = [1, 2, 31, 32, 33, 255, 256, 257, GT - 1, GT, GT + 1,
               2 * GT + 5, R.GRP_SCAN * GT, R.GRP_SCAN * GT + 1,
               (R.GRP_SCAN + 1) * GT + 3]


def _geometric_runs(n, rng):
    lens = np.append(rng.geometric(1 / 20, n // 8 + 2), n)   # sum >= n
    lens = lens[:np.searchsorted(np.cumsum(lens), n) + 1]
    gaps = rng.integers(1, 1 << 40, len(lens)).astype(np.uint64)
    return np.repeat(np.cumsum(gaps), lens)[:n]


def _three_tile_run(n, rng):
    k = np.arange(n, dtype=np.uint64) * np.uint64(2)
    a, b = (GT - 5, 3 * GT + 7) if n > 3 * GT + 8 else (n // 3, 2 * n // 3)
    if b > a:
        k[a:b] = k[a]
    return k


def _extremes(n, rng):
    k = _geometric_runs(n, rng)
    k[:min(n, 40)] = 0
    k[max(0, n - 33):] = ONES
    return k


GROUP_PATTERNS = {
    "all-equal": lambda n, rng: np.full(n, 0x5555555555555555, np.uint64),
    "all-distinct": lambda n, rng:
        np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(7),
    "runs-of-32-aligned": lambda n, rng:
        np.arange(n, dtype=np.uint64) // np.uint64(32) * np.uint64(5),
    "runs-of-32-shifted-by-31": lambda n, rng:
        (np.arange(n, dtype=np.uint64) + np.uint64(1)) // np.uint64(32),
    "boundaries-on-tile-edges-only": lambda n, rng:
        np.arange(n, dtype=np.uint64) // np.uint64(GT) * BIG,
    "one-run-over-three-tiles": _three_tile_run,
    "first-0-last-all-ones": _extremes,
    "geometric-runs": _geometric_runs,
}


@pytest.mark.parametrize("pattern", list(GROUP_PATTERNS))
def test_group_index_size_ladder(nat, stream, pattern):
    rng = np.random.default_rng(len(pattern))
    for n in GROUP_SIZES:
        keys = GROUP_PATTERNS[pattern](n, rng)
        assert len(keys) == n and np.all(keys[1:] >= keys[:-1])
        eu, eo = R.group_index(keys)
        din = U.In(keys)
        du, do = U.Out(n, np.uint64), U.Out(n, np.uint64)
        dc = U.garbage(1, np.uint64)
        w = U.filled_ws(nat.ws("group_index", n))
        nat.group_index(din.ptr, n, du.ptr, do.ptr, dc.data_ptr(),
                        w.data_ptr(), stream)
        U.sync()
        m = int(U.G.host(dc, np.uint64)[0])
        assert m == len(eu), (n, m, len(eu))
        assert np.array_equal(du.read(valid=m), eu), n
        assert np.array_equal(do.read(valid=m), eo), n
        din.check()


# -------------------------------------------------------------- merge_u64

MT = R.MRG_TILE
MERGE_SIZES = [(1, 1), (1, MT - 1), (MT - 1, 1), (MT // 2, MT // 2),
               (MT, MT), (MT + 1, MT - 1), (3, 2 * MT - 2), (10000, 13),
               (3 * MT + 1, 3 * MT + 2)]
EIGHT = np.array([0, 1, 1 << 31, 1 << 32, (1 << 63) - 1, 1 << 63,
                  0xFFFFFFFFFFFFFFFE, 0xFFFFFFFFFFFFFFFF], np.uint64)


def _tile_blocks(n, odd):
    """block i of MRG_TILE consecutive keys sits in slot 2i (+1 if odd) of
    the merged order: every full output tile is fed from one input."""
    i = np.arange(n, dtype=np.uint64)
    t = np.uint64(MT)
    return (i // t * np.uint64(2) + np.uint64(odd)) * BIG + i % t


def _with_extremes(x):
    x = np.sort(x)
    x[0] = 0
    x[-1] = ONES        # a single element ends up as 2^64-1
    return x


MERGE_PATTERNS = {
    "random-distinct": lambda na, nb, rng:
        (np.sort(rand_u64(rng, na)), np.sort(rand_u64(rng, nb))),
    "a-below-b": lambda na, nb, rng:
        (np.sort(rand_u64(rng, na) >> np.uint64(2)),
         np.sort(rand_u64(rng, nb) | np.uint64(1 << 63))),
    "a-above-b": lambda na, nb, rng:
        (np.sort(rand_u64(rng, na) | np.uint64(1 << 63)),
         np.sort(rand_u64(rng, nb) >> np.uint64(2))),
    "eight-values": lambda na, nb, rng:
        (np.sort(rng.choice(EIGHT, na)), np.sort(rng.choice(EIGHT, nb))),
    "alternating-tile-blocks": lambda na, nb, rng:
        (_tile_blocks(na, 0), _tile_blocks(nb, 1)),
    "both-hold-0-and-all-ones": lambda na, nb, rng:
        (_with_extremes(rand_u64(rng, na)),
         _with_extremes(rng.choice(EIGHT, nb))),
}


@pytest.mark.parametrize("pattern", list(MERGE_PATTERNS))
def test_merge_u64_tile_and_span_edges(nat, stream, pattern):
    # Equal keys from A and from B are the same 64 bits, so neither the
    # A-before-B rule nor a disagreement about it between the block-level
    # and the thread-level search can be observed here: every tie rule
    # yields a valid merge-path split, and a span that starts from another
    # valid split than its neighbour ended on emits equal keys of A in
    # place of as many equal keys of B. What these shapes check is that
    # the searches' bounds, the LDS staging and the span ends hold where
    # runs of equals, one-sided tiles and partial tiles meet the tile and
    # the 16-element span edges: a search that returns an INVALID split
    # loses and duplicates keys of different value.
    rng = np.random.default_rng(len(pattern))
    for na, nb in MERGE_SIZES:
        a, b = MERGE_PATTERNS[pattern](na, nb, rng)
        assert len(a) == na and len(b) == nb
        assert np.all(a[1:] >= a[:-1]) and np.all(b[1:] >= b[:-1])
        da, db = U.In(a), U.In(b)
        out = U.Out(na + nb, np.uint64)
        nat.merge_u64(da.ptr, na, db.ptr, nb, out.ptr, stream)
        U.sync()
        assert np.array_equal(out.read(), R.merge(a, b)), (na, nb)
        da.check()
        db.check()


# ---------------------------------------------------------- merge_records

RT = R.MRG_REC_TILE
MERGE_REC_SIZES = [(1, 1), (1, RT - 1), (RT // 2, RT // 2), (RT, RT),
                   (RT + 1, RT - 1), (5000, 3)]


def _pool16(n, rec, rng):
    pool = rng.integers(0, 256, (16, rec)).astype(np.uint8)
    pool[:, 0] = np.arange(16) * 17          # 16 distinct records
    return pool[rng.integers(0, 16, n)]


def _last_byte(n, rec, rng):
    r = np.tile(rng.integers(0, 256, rec).astype(np.uint8), (n, 1))
    r[:, rec - 1] = (np.arange(n) * 37 + rng.integers(0, 256)) % 256
    return r


def _byte0_vs_byte3(n, rec, rng):
    """all records share every byte but bytes 0 and 3 of one word: byte 0
    decides first in byte order, byte 3 in a word compare without swap."""
    r = np.tile(rng.integers(0, 256, rec).astype(np.uint8), (n, 1))
    w = 4 * ((rec // 4) // 2)
    r[:, w] = rng.integers(0, 3, n)
    r[:, w + 3] = rng.integers(0, 256, n)
    return r


MERGE_REC_PATTERNS = {
    "pool-of-16": _pool16,
    "last-byte-only": _last_byte,
    "byte0-vs-byte3": _byte0_vs_byte3,
    "random-bytes": lambda n, rec, rng:
        rng.integers(0, 256, (n, rec)).astype(np.uint8),
}


@pytest.mark.parametrize("pattern", list(MERGE_REC_PATTERNS))
@pytest.mark.parametrize("rec", [4, 8, 12, 100, 128])
def test_merge_records_tile_and_span_edges(nat, stream, rec, pattern):
    # as for merge_u64: equal records are identical bytes, so the tie rule
    # cannot be observed; the byte order of the compare can
    rng = np.random.default_rng(rec * 31 + len(pattern))
    gen = MERGE_REC_PATTERNS[pattern]
    for na, nb in MERGE_REC_SIZES:
        # both inputs draw from ONE family of records, so that equal and
        # nearly equal records meet across A and B
        both = gen(na + nb, rec, rng)
        A, B = R.sort_records(both[:na]), R.sort_records(both[na:])
        da, db = U.In(A), U.In(B)
        out = U.Out((na + nb) * rec, np.uint8)
        nat.merge_records(da.ptr, na, db.ptr, nb, rec, out.ptr, stream)
        U.sync()
        got = out.read().reshape(na + nb, rec)
        assert np.array_equal(got, R.merge_records(A, B)), (na, nb)
        da.check()
        db.check()


# ----------------------------------------------------------- classify_u64

CG = R.CLASSIFY_GRID_CAP * 256            # items per trip of the full grid
# (n, p): every p at the sizes up to one full trip; past it the reference
# costs n * p, so the second and third trips run with p <= 8
CLASSIFY_CASES = [(n, p) for n in (1, 255, 256, 257, CG)
                  for p in (1, 2, 255, 256)] + \
                 [(n, p) for n in (CG + 1, 2 * CG + 3) for p in (1, 2, 8)]


def sample_splitters(keys, gidx0, p, rng, extra_idx=()):
    """p-1 items (key, global index) sampled from the input itself, first
    and last item included when they fit, sorted by (key, index): each
    splitter equals one item exactly, index and all."""
    m = p - 1
    pos = rng.integers(0, len(keys), m)
    pos[:min(m, 2)] = [0, len(keys) - 1][:min(m, 2)]
    sk = keys[pos]
    si = pos.astype(np.uint64) + np.uint64(gidx0)
    for j, g in enumerate(extra_idx[:m]):
        si[m - 1 - j] = g
    order = np.lexsort((si, sk))
    return sk[order], si[order]


def _cls_dup_heavy(n, p, rng):
    keys = rng.integers(0, 16, n).astype(np.uint64) * np.uint64(1 << 59)
    return (keys, 12345) + sample_splitters(keys, 12345, p, rng)


def _cls_one_key(n, p, rng):
    # all items and all splitters share one key: the index alone decides;
    # some splitter indices lie before and behind the items' range
    keys = np.full(n, 0x0123456789ABCDEF, np.uint64)
    g0 = 1000
    return (keys, g0) + sample_splitters(
        keys, g0, p, rng, extra_idx=(0, g0 - 1, g0 + n, g0 + n + 7))


def _cls_gidx_2_40(n, p, rng):
    # global indices above 2^32; two splitters just below 2^40, whose low
    # 32 bits are larger than every item's
    keys = rng.integers(0, 4, n).astype(np.uint64)
    g0 = 1 << 40
    return (keys, g0) + sample_splitters(
        keys, g0, p, rng, extra_idx=(g0 - 1, g0 - 5))


def _cls_own_index(n, p, rng):
    keys = rng.integers(0, 3, n).astype(np.uint64) * np.uint64(1 << 62)
    return (keys, 0) + sample_splitters(keys, 0, p, rng)


def _cls_extremes(n, p, rng):
    keys = rng.choice(np.array([0, ONES], np.uint64), n)
    keys[-1] = ONES                       # a splitter with key 2^64-1
    return (keys, 77) + sample_splitters(keys, 77, p, rng)


CLASSIFY_PATTERNS = {
    "duplicate-heavy": _cls_dup_heavy,
    "one-key-index-decides": _cls_one_key,
    "gidx0-2^40": _cls_gidx_2_40,
    "splitter-is-the-item": _cls_own_index,
    "keys-0-and-all-ones": _cls_extremes,
}


@pytest.mark.parametrize("pattern", list(CLASSIFY_PATTERNS))
def test_classify_u64_grid_trips_and_tie_break(nat, oracle, stream, pattern):
    rng = np.random.default_rng(len(pattern))
    for n, p in CLASSIFY_CASES:
        keys, g0, sk, si = CLASSIFY_PATTERNS[pattern](n, p, rng)
        exp = R.classify(keys, g0, sk, si)
        assert np.array_equal(exp, oracle.classify_u64(keys, g0, sk, si, p))
        cnt = np.bincount(exp, minlength=p).astype(np.uint64)
        dk, dsk, dsi = U.In(keys), U.In(sk), U.In(si)
        dc = U.garbage(p + U.NCAN, np.uint64)
        for _ in range(2):                # the call zeroes d_counts itself
            db = U.Out(n, np.uint32)
            nat.classify_u64(dk.ptr, n, g0, dsk.ptr, dsi.ptr, p, db.ptr,
                             dc.data_ptr(), stream)
            U.sync()
            assert np.array_equal(db.read(), exp), (n, p)
            c = U.G.host(dc, np.uint64)
            assert np.array_equal(c[:p], cnt), (n, p)
            assert np.all(c[p:] == U.CANARY[np.uint64]), (n, p)
        for d in (dk, dsk, dsi):
            d.check()


# ----------------------------------------------------------- classify_rec

def _rec_last_byte(n, rec, rng):
    r = np.tile(rng.integers(0, 256, rec).astype(np.uint8), (n, 1))
    r[:, rec - 1] = rng.integers(0, 256, n)
    return r


def _rec_high_bytes(n, rec, rng):
    pool = rng.choice(np.array([0x00, 0x7F, 0x80, 0xFF], np.uint8),
                      (32, rec))
    pool[:16, :8] = pool[0, :8]            # half share the u64 prefix
    return pool[rng.integers(0, 32, n)]


def _rec_three(n, rec, rng):
    pool = rng.integers(0, 256, (3, rec)).astype(np.uint8)
    pool[1] = pool[0]
    pool[1, rec - 1] ^= 0x80
    return pool[rng.integers(0, 3, n)]


CLASSIFY_REC_PATTERNS = {
    "differ-in-the-last-byte": _rec_last_byte,
    "bytes-at-and-above-0x80": _rec_high_bytes,
    "items-equal-to-splitters": _rec_three,
}


@pytest.mark.parametrize("pattern", list(CLASSIFY_REC_PATTERNS))
@pytest.mark.parametrize("rec", [8, 12, 100])
def test_classify_rec_byte_fallback_and_tie_break(nat, oracle, stream, rec,
                                                  pattern):
    rng = np.random.default_rng(rec * 7 + len(pattern))
    g0 = (1 << 40) + 11
    for n, p in [(1, 256), (257, 256), (CG + 1, 8)]:
        recs = CLASSIFY_REC_PATTERNS[pattern](n, rec, rng)
        m = p - 1
        pos = rng.integers(0, n, m)
        pos[:2] = [0, n - 1]
        spl, si = recs[pos], pos.astype(np.uint64) + np.uint64(g0)
        order = np.lexsort((si,) + tuple(spl[:, j]
                                         for j in range(rec - 1, -1, -1)))
        spl, si = np.ascontiguousarray(spl[order]), si[order]
        exp = R.classify_rec(recs, g0, spl, si)
        assert np.array_equal(
            exp, oracle.classify_rec(recs, g0, rec, spl, si, p))
        cnt = np.bincount(exp, minlength=p).astype(np.uint64)
        ins = [U.In(recs), U.In(be_prefix(recs)), U.In(spl),
               U.In(be_prefix(spl)), U.In(si)]
        dc = U.garbage(p + U.NCAN, np.uint64)
        for _ in range(2):
            db = U.Out(n, np.uint32)
            nat.classify_rec(ins[0].ptr, ins[1].ptr, n, g0, ins[2].ptr,
                             ins[3].ptr, ins[4].ptr, p, rec, db.ptr,
                             dc.data_ptr(), stream)
            U.sync()
            assert np.array_equal(db.read(), exp), (n, p)
            c = U.G.host(dc, np.uint64)
            assert np.array_equal(c[:p], cnt), (n, p)
            assert np.all(c[p:] == U.CANARY[np.uint64]), (n, p)
        for d in ins:
            d.check()


# ---------------------------------------------------------- partition_idx

PT = R.PAIRS_TILE
PART_SIZES = [1, 255, 256, 257, PT - 1, PT, PT + 1, R.SCAN_CHUNK * PT,
              R.SCAN_CHUNK * PT + 1,
              R.CHUNKSCAN_UNROLL * R.SCAN_CHUNK * PT + 5]

PART_PATTERNS = {
    "all-0": lambda n, p, rng: np.zeros(n, np.uint32),
    "all-last": lambda n, p, rng: np.full(n, p - 1, np.uint32),
    "odd-only": lambda n, p, rng:
        (rng.integers(0, max(p // 2, 1), n) * 2 + 1).clip(0, p - 1),
    "i-mod-p": lambda n, p, rng: np.arange(n) % p,
    "descending": lambda n, p, rng: (p - 1) - np.arange(n) * p // n,
    "random": lambda n, p, rng: rng.integers(0, p, n),
}


@pytest.mark.parametrize("pattern", list(PART_PATTERNS))
@pytest.mark.parametrize("p", [1, 2, 255, 256])
def test_partition_idx_tiles_chunks_and_empty_buckets(nat, stream, p,
                                                      pattern):
    rng = np.random.default_rng(p * 13 + len(pattern))
    for n in PART_SIZES:
        bucket = PART_PATTERNS[pattern](n, p, rng).astype(np.uint32)
        assert len(bucket) == n and bucket.max() < p
        perm, off = R.partition(bucket, p)
        assert off[0] == 0 and off[p] == n and len(off) == p + 1
        din = U.In(bucket)
        dp, do = U.Out(n, np.uint32), U.Out(p + 1, np.uint64)
        w = U.filled_ws(nat.ws("partition_idx", n))
        nat.partition_idx(din.ptr, n, p, dp.ptr, do.ptr, w.data_ptr(),
                          stream)
        U.sync()
        assert np.array_equal(do.read(), off), n
        assert np.array_equal(dp.read(), perm), n
        din.check()


# --------------------------------------------------------- gather_records

def gather_indices(n, rng):
    """(name, idx, number of source records)"""
    yield "permutation", rng.permutation(n), n
    yield "identity", np.arange(n), n
    yield "reversed", np.arange(n)[::-1], n
    yield "broadcast", np.full(n, n // 2), n
    yield "repeats", rng.integers(0, 2 * n, n), 2 * n


def check_gather(nat, stream, rec, sizes, seed):
    rng = np.random.default_rng(seed)
    for n in sizes:
        for name, idx, nsrc in gather_indices(n, rng):
            src = rng.integers(0, 256, (nsrc, rec), dtype=np.uint8)
            idx = np.ascontiguousarray(idx, dtype=np.uint32)
            ds, di = U.In(src), U.In(idx)
            out = U.Out(n * rec, np.uint8)
            nat.gather_records(ds.ptr, di.ptr, n, rec, out.ptr, stream)
            U.sync()
            assert np.array_equal(out.read().reshape(n, rec), src[idx]), \
                (rec, n, name)
            ds.check()
            di.check()


GATHER_SIZES = [1, 2, 3, 41, 1000]
# 100-byte records, more words than 16384 blocks of 4 x 256 cover
GATHER_BIG = 170_001
assert GATHER_BIG * 25 > R.RECORDS_GRID_CAP * 256


@pytest.mark.parametrize("rec", [4, 8, 12, 128])
def test_gather_records_default_variant(nat, stream, rec, monkeypatch):
    monkeypatch.delenv("T9_GATHER_VARIANT", raising=False)
    check_gather(nat, stream, rec, GATHER_SIZES, rec)


@pytest.mark.parametrize("variant", [None, 1, 2, 4])
def test_gather_records_100_byte_variants(nat, stream, variant,
                                          monkeypatch):
    # the variable is read on every call; None is the default span kernel
    if variant is None:
        monkeypatch.delenv("T9_GATHER_VARIANT", raising=False)
    else:
        monkeypatch.setenv("T9_GATHER_VARIANT", str(variant))
    check_gather(nat, stream, 100, GATHER_SIZES + [GATHER_BIG],
                 100 + (variant or 0))


# ------------------------------------------------ extract_key64 (BE, LE)

EXTRACT_SIZES = [1, 257, 10_001]
EXTRACT_BIG = R.RECORDS_GRID_CAP * 256 + 3     # second grid-stride trip


@pytest.mark.parametrize("le", [False, True], ids=["be", "le"])
@pytest.mark.parametrize("rec,key_off", [(8, 0), (12, 0), (12, 4), (100, 0),
                                         (100, 4), (100, 92), (128, 8),
                                         (128, 120)])
def test_extract_key64_offsets_and_paths(nat, stream, rec, key_off, le):
    # LE reads one aligned u64 when rec and key_off allow it — (8, 0),
    # (128, 8), (128, 120) — and two u32 words otherwise; both against the
    # same view of the bytes
    rng = np.random.default_rng(rec * 131 + key_off)
    sizes = EXTRACT_SIZES + ([EXTRACT_BIG] if (rec, key_off) in
                             ((8, 0), (12, 4)) else [])
    fn = nat.extract_key64_le if le else nat.extract_key64
    for n in sizes:
        recs = rng.integers(0, 256, (n, rec), dtype=np.uint8)
        exp = recs[:, key_off:key_off + 8].copy().view(
            "<u8" if le else ">u8").ravel().astype(np.uint64)
        din = U.In(recs)
        dk, di = U.Out(n, np.uint64), U.Out(n, np.uint32)
        fn(din.ptr, n, rec, key_off, dk.ptr, di.ptr, stream)
        U.sync()
        assert np.array_equal(dk.read(), exp), n
        assert np.array_equal(di.read(), np.arange(n, dtype=np.uint32)), n
        din.check()
