"""GPU tests of the chunked sort -> gather pipeline of the record sort
(sort_msb_impl, 9-bit two-level flow): the sub-bucket sort of chunk c + 1
runs on the caller's stream while the internal stream gathers the records
of chunk c. Every case is compared byte for byte against the CPU oracle
AND against the same call with T9_SORT_OVERLAP=0, and asserts through
t9_sort_last_schedule that the schedule it meant to exercise really ran.
The overlapped schedule is off by default (measured slower), so
the module enables it with T9_SORT_OVERLAP=1.

Sub-bucket of a record = top 17 bits of its big-endian 8-byte prefix
(256 x 512 = NSUB9 sub-buckets); chunk c of K covers the sub-buckets
[c * NSUB9 // K, (c + 1) * NSUB9 // K)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tests import _gpu as G
    from thrill_amd import Native

NSUB9 = 256 * 512
DEFAULT_K = 8


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = Native(device=0)
    yield n
    n.close()


@pytest.fixture(autouse=True)
def msb_env():
    saved = {k: os.environ.get(k) for k in
             ("T9_SORT_ALGO", "T9_SORT_OVERLAP", "T9_SORT_OVERLAP_CHUNKS",
              "T9_PASS2_BITS", "T9_MSB_LEVELS", "T9_EXTRACT_IOTA")}
    os.environ["T9_SORT_ALGO"] = "msb"
    os.environ["T9_SORT_OVERLAP"] = "1"
    for k in list(saved)[2:]:
        os.environ.pop(k, None)
    yield
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def prefixes(recs):
    return recs[:, :8].copy().view(">u8").reshape(-1).astype(np.uint64)


def chunks_hit(recs, K):
    """number of non-empty chunks for these records at K chunks"""
    sub = (prefixes(recs) >> np.uint64(47)).astype(np.int64)
    edges = np.array([c * NSUB9 // K for c in range(1, K)], dtype=np.int64)
    return len(np.unique(np.searchsorted(edges, sub, side="right")))


def chunk_of(recs, K):
    sub = (prefixes(recs) >> np.uint64(47)).astype(np.int64)
    edges = np.array([c * NSUB9 // K for c in range(1, K)], dtype=np.int64)
    return np.searchsorted(edges, sub, side="right")


def gpu_sort(nat, recs, keyle=False):
    n, rs = recs.shape
    din = G.dev(recs.reshape(-1))
    dout = G.empty(n * rs, np.uint8)
    w = G.ws(nat.ws("sort_records", n, rs))
    if keyle:
        nat.sort_records_keyle(G.ptr(din), G.ptr(dout), n, rs, G.ptr(w),
                               G.stream())
    else:
        nat.sort_records(G.ptr(din), G.ptr(dout), n, rs, min(10, rs),
                         G.ptr(w), G.stream())
    got = G.host(dout, np.uint8).reshape(n, rs)
    assert np.array_equal(G.host(din, np.uint8).reshape(n, rs), recs), \
        "input not preserved"
    return got, nat.sort_last_schedule()


def both_schedules(nat, recs, keyle=False):
    """(output, schedule) of the T9_SORT_OVERLAP=1 run; the
    T9_SORT_OVERLAP=0 run must be serial and byte-identical."""
    got, sched = gpu_sort(nat, recs, keyle)
    os.environ["T9_SORT_OVERLAP"] = "0"
    try:
        ser, s0 = gpu_sort(nat, recs, keyle)
    finally:
        os.environ["T9_SORT_OVERLAP"] = "1"
    assert s0 == 0
    assert np.array_equal(got, ser), "overlapped != serial"
    return got, sched


_uniform = {}


def uniform(oracle, n):
    """seeded uniform records + their oracle order, computed once (tests
    that plant duplicates work on a copy)"""
    if n not in _uniform:
        recs = oracle.gen_records(n, seed=0x0513 + n)
        exp = oracle.sort_records(recs)
        exp.setflags(write=False)
        _uniform[n] = (recs, exp)
    return _uniform[n]


# ---- 1. uniform prefixes: overlapped at every K ----------------------

@pytest.mark.parametrize("K", [2, 4, 16])
@pytest.mark.parametrize("n", [(1 << 14) + 1, (1 << 17) + 3, 1 << 20])
def test_uniform_overlapped(nat, oracle, n, K):
    recs, exp = uniform(oracle, n)
    assert len(np.unique(prefixes(recs))) == n, "seed has equal prefixes"
    os.environ["T9_SORT_OVERLAP_CHUNKS"] = str(K)
    got, sched = both_schedules(nat, recs)
    assert sched == chunks_hit(recs, K) and sched >= 1
    assert np.array_equal(got, exp)


def test_uniform_default_chunks(nat, oracle):
    recs, exp = uniform(oracle, (1 << 17) + 3)
    got, sched = both_schedules(nat, recs)
    assert sched == DEFAULT_K
    assert np.array_equal(got, exp)


def test_default_is_serial(nat, oracle):
    recs, exp = uniform(oracle, (1 << 17) + 3)
    del os.environ["T9_SORT_OVERLAP"]
    got, sched = gpu_sort(nat, recs)
    assert sched == 0
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("rs", [100, 128])
def test_extract_iota_knob_parity(nat, oracle, rs):
    """the pass-1 scatter makes the index iota itself (default); writing
    it in the extract and reading it back (T9_EXTRACT_IOTA=1) must give
    the same bytes, on either schedule"""
    n = (1 << 16) + 11
    rng = np.random.default_rng(rs)
    recs = rng.integers(0, 256, (n, rs)).astype(np.uint8)
    got, _ = both_schedules(nat, recs)
    os.environ["T9_EXTRACT_IOTA"] = "1"
    old, _ = both_schedules(nat, recs)
    assert np.array_equal(got, old)
    assert np.array_equal(got, oracle.sort_records(recs))


# ---- 2. every key inside one chunk's sub-bucket range ----------------

@pytest.mark.parametrize("top", [0x00, 0xFF])
def test_single_chunk(nat, oracle, top):
    # 2^17 records over the 512 sub-buckets of one top byte: ~256 each
    n = 1 << 17
    recs = oracle.gen_records(n, seed=0x77 + top).copy()
    recs[:, 0] = top
    sub = prefixes(recs) >> np.uint64(47)
    assert np.bincount((sub & np.uint64(511)).astype(np.int64)).max() <= 1024
    got, sched = both_schedules(nat, recs)
    assert sched == 1
    assert np.array_equal(got, oracle.sort_records(recs))


# ---- 3. duplicated prefixes: overlap starts, tie path takes over -----

@pytest.mark.parametrize("where", ["first", "last", "every"])
def test_duplicate_prefix(nat, oracle, where):
    n = 1 << 17
    recs = uniform(oracle, n)[0].copy()
    ch = chunk_of(recs, DEFAULT_K)
    want = {"first": [0], "last": [DEFAULT_K - 1],
            "every": list(range(DEFAULT_K))}[where]
    for c in want:
        i, j = np.flatnonzero(ch == c)[:2]     # i < j, same chunk
        recs[j, :8] = recs[i, :8]
        # the stable pair sort leaves (i, j); full-record order is (j, i),
        # so only the tie machinery + re-gather can produce the output
        recs[i, 8] = 0xFF
        recs[j, 8] = 0x00
    got, sched = both_schedules(nat, recs)
    assert sched == DEFAULT_K, "overlapped schedule did not start"
    exp = oracle.sort_records(recs)
    assert np.array_equal(got, exp)
    # ordered by the full record bytes (lexsort is stable: identity iff
    # already sorted)
    order = np.lexsort(tuple(got[:, c] for c in range(99, -1, -1)))
    assert np.array_equal(order, np.arange(n))


# ---- 4. inputs that must take the serial schedule --------------------

def planted(oracle, n, m):
    """uniform records, the first m forced into one sub-bucket"""
    recs = oracle.gen_records(n, seed=0x4A + m).copy()
    recs[:m, 0] = 0x5A
    recs[:m, 1] = 0xC3
    recs[:m, 2] &= 0x7F
    return recs


@pytest.mark.parametrize("m", [1100, 5000])
def test_serial_oversize_sub_bucket(nat, oracle, m):
    # 1100 > wave16 tier (1024): maxsub too large; 5000 > T9_SUBMAX (4096):
    # oversize list non-empty
    recs = planted(oracle, 1 << 17, m)
    got, sched = both_schedules(nat, recs)
    assert sched == 0
    assert np.array_equal(got, oracle.sort_records(recs))


def test_serial_all_identical(nat, oracle):
    n = 1 << 15
    recs = np.repeat(oracle.gen_records(1, seed=9), n, axis=0)
    got, sched = both_schedules(nat, recs)
    assert sched == 0
    assert np.array_equal(got, recs)


@pytest.mark.parametrize("var,val", [("T9_PASS2_BITS", "8"),
                                     ("T9_MSB_LEVELS", "3")])
def test_serial_other_flows(nat, oracle, var, val):
    recs, exp = uniform(oracle, (1 << 17) + 3)
    os.environ[var] = val
    got, sched = both_schedules(nat, recs)
    assert sched == 0
    assert np.array_equal(got, exp)


def test_serial_perf_timing(nat, oracle):
    recs, exp = uniform(oracle, (1 << 17) + 3)
    nat.perf_reset()
    nat.perf_enable(True)
    try:
        got, sched = gpu_sort(nat, recs)
        torch.cuda.synchronize()
        _, launches = nat.perf_read("gather")
    finally:
        nat.perf_enable(False)
        nat.perf_reset()
    assert sched == 0
    assert launches == 1
    assert np.array_equal(got, exp)


def test_serial_128_byte_records(nat, oracle):
    n = 1 << 15
    rng = np.random.default_rng(31)
    recs = rng.integers(0, 256, (n, 128)).astype(np.uint8)
    got, sched = both_schedules(nat, recs)
    assert sched == 0
    assert np.array_equal(got, oracle.sort_records(recs))


def test_keyle_100_byte_is_overlapped(nat):
    # 100-byte records with a little-endian key go through the same fused
    # extract + 9-bit flow, so they ARE eligible: overlapped, with parity
    n = (1 << 15) + 5
    rng = np.random.default_rng(41)
    recs = rng.integers(0, 256, (n, 100)).astype(np.uint8)
    got, sched = both_schedules(nat, recs, keyle=True)
    assert sched == DEFAULT_K
    keys = recs[:, :8].copy().view("<u8").reshape(-1)
    order = np.lexsort(tuple(recs[:, c] for c in range(99, 7, -1))
                       + (keys,))
    assert np.array_equal(got, recs[order])


def test_keyle_128_byte_is_serial(nat):
    n = 1 << 15
    rng = np.random.default_rng(43)
    recs = rng.integers(0, 256, (n, 128)).astype(np.uint8)
    got, sched = both_schedules(nat, recs, keyle=True)
    assert sched == 0
    keys = recs[:, :8].copy().view("<u8").reshape(-1)
    order = np.lexsort(tuple(recs[:, c] for c in range(127, 7, -1))
                       + (keys,))
    assert np.array_equal(got, recs[order])


# ---- 5. one context, three sorts, two streams, then close ------------

def test_context_reuse_across_streams(oracle):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    nat = Native(device=0)
    try:
        side = torch.cuda.Stream()
        plan = [((1 << 16) + 7, 0x101, None), ((1 << 17) + 1, 0x202, side),
                ((1 << 14) + 9, 0x303, None)]
        for n, seed, st in plan:
            recs = oracle.gen_records(n, seed=seed)
            if st is None:
                got, sched = gpu_sort(nat, recs)
            else:
                torch.cuda.synchronize()
                with torch.cuda.stream(st):
                    got, sched = gpu_sort(nat, recs)
                st.synchronize()
            assert sched == chunks_hit(recs, DEFAULT_K) and sched >= 1
            assert np.array_equal(got, oracle.sort_records(recs))
    finally:
        nat.close()
