"""GPU tests of the fused sub-bucket sort + payload gather of the record
sort (k_wave16_sort_gather, 9-bit two-level flow, 100-byte records): each
single-wave block sorts its sub-bucket and then copies that sub-bucket's
records itself. Every case is compared byte for byte against the CPU oracle
AND against the same call with T9_SORT_FUSED_GATHER=0, asserts through
t9_sort_last_fused which path ran (1 = the fused kernel produced the
output, 2 = it started but ties forced the redo, 0 = separate kernels) and
that the input is unchanged. The module asks for the fused path with
T9_SORT_FUSED_GATHER=1, so the cases hold whatever the library's default.

Sub-bucket of a record = top 17 bits of its big-endian 8-byte prefix
(256 x 512 = NSUB9 sub-buckets). Equal-prefix runs of up to 8 records are
settled inside the block (fused = 1); longer runs and a sub-bucket whose
keys are all equal go to the tie path (fused = 2)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tests import _gpu as G
    from thrill_amd import Native

NSUB9 = 256 * 512
GUARD = 4096
SENTINEL = 0xA5
KNOBS = ("T9_SORT_ALGO", "T9_SORT_FUSED_GATHER", "T9_SORT_OVERLAP",
         "T9_SORT_OVERLAP_CHUNKS", "T9_PASS2_BITS", "T9_MSB_LEVELS",
         "T9_GATHER_VARIANT", "T9_EXTRACT_IOTA")


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = Native(device=0)
    yield n
    n.close()


@pytest.fixture(autouse=True)
def fused_env():
    saved = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ["T9_SORT_ALGO"] = "msb"
    os.environ["T9_SORT_FUSED_GATHER"] = "1"
    yield
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def prefixes(recs):
    return recs[:, :8].copy().view(">u8").reshape(-1).astype(np.uint64)


def subs_of(recs):
    return (prefixes(recs) >> np.uint64(47)).astype(np.int64)


def gpu_sort(nat, recs, keyle=False, guards=False):
    """-> (output, t9_sort_last_fused); d_out sits between two sentinel
    guards when asked, and both are checked"""
    n, rs = recs.shape
    din = G.dev(recs.reshape(-1))
    if guards:
        buf = torch.full((n * rs + 2 * GUARD,), SENTINEL, dtype=torch.uint8,
                         device="cuda")
        dout = buf[GUARD:GUARD + n * rs]
    else:
        dout = G.empty(n * rs, np.uint8)
    w = G.ws(nat.ws("sort_records", n, rs))
    if keyle:
        nat.sort_records_keyle(G.ptr(din), G.ptr(dout), n, rs, G.ptr(w),
                               G.stream())
    else:
        nat.sort_records(G.ptr(din), G.ptr(dout), n, rs, min(10, rs),
                         G.ptr(w), G.stream())
    got = G.host(dout, np.uint8).reshape(n, rs).copy()
    assert np.array_equal(G.host(din, np.uint8).reshape(n, rs), recs), \
        "input not preserved"
    if guards:
        h = G.host(buf, np.uint8)
        assert (h[:GUARD] == SENTINEL).all(), "front guard overwritten"
        assert (h[GUARD + n * rs:] == SENTINEL).all(), \
            "back guard overwritten"
    return got, nat.sort_last_fused()


def both(nat, recs, keyle=False, guards=False):
    """(output, fused) of the T9_SORT_FUSED_GATHER=1 run; the =0 run must
    take the separate kernels and be byte-identical"""
    got, fused = gpu_sort(nat, recs, keyle, guards)
    os.environ["T9_SORT_FUSED_GATHER"] = "0"
    try:
        ser, f0 = gpu_sort(nat, recs, keyle, guards)
    finally:
        os.environ["T9_SORT_FUSED_GATHER"] = "1"
    assert f0 == 0
    assert np.array_equal(got, ser), "fused != separate kernels"
    return got, fused


_uniform = {}


def uniform(oracle, n):
    """seeded uniform records + their oracle order, computed once (tests
    that plant records work on a copy)"""
    if n not in _uniform:
        recs = oracle.gen_records(n, seed=0x0F17 + n)
        assert len(np.unique(prefixes(recs))) == n, "seed has equal prefixes"
        exp = oracle.sort_records(recs)
        exp.setflags(write=False)
        _uniform[n] = (recs, exp)
    return _uniform[n]


def assert_fully_ordered(got):
    """ordered by the full record bytes (lexsort is stable: identity iff
    already sorted)"""
    order = np.lexsort(tuple(got[:, c] for c in range(got.shape[1] - 1, -1,
                                                      -1)))
    assert np.array_equal(order, np.arange(len(got)))


# ---- 1. uniform prefixes ---------------------------------------------

@pytest.mark.parametrize("n", [(1 << 14) + 1, (1 << 17) + 3, 1 << 20])
def test_uniform(nat, oracle, n):
    # 2^14+1: nearly every sub-bucket holds 0 or 1 record (the ns <= 1
    # copy); 2^17+3: sizes 0..6; 2^20: about 8 each
    recs, exp = uniform(oracle, n)
    got, fused = both(nat, recs)
    assert fused == 1
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("n", [(1 << 14) + 1, (1 << 17) + 3])
def test_guard_bytes(nat, oracle, n):
    recs, exp = uniform(oracle, n)
    got, fused = both(nat, recs, guards=True)
    assert fused == 1
    assert np.array_equal(got, exp)


# ---- 2. the full 1024 tier --------------------------------------------

def planted(oracle, n, m):
    """uniform records, exactly the first m in one sub-bucket"""
    recs = oracle.gen_records(n, seed=0x4A + m).copy()
    recs[:m, 0] = 0x5A
    recs[:m, 1] = 0xC3
    recs[:m, 2] &= 0x7F
    sub = subs_of(recs)
    stray = np.flatnonzero(sub[m:] == sub[0]) + m
    recs[stray, 0] = 0x5B
    assert np.count_nonzero(subs_of(recs) == sub[0]) == m
    assert len(np.unique(prefixes(recs))) == n
    return recs


@pytest.mark.parametrize("m,want", [(1023, 1), (1024, 1), (1025, 0)])
def test_full_tier(nat, oracle, m, want):
    recs = planted(oracle, 1 << 17, m)
    got, fused = both(nat, recs)
    assert fused == want
    assert np.array_equal(got, oracle.sort_records(recs))


def test_one_top_byte(nat, oracle):
    # 2^17 records over the 512 sub-buckets of one top byte: ~256 each
    n = 1 << 17
    recs = oracle.gen_records(n, seed=0x77).copy()
    recs[:, 0] = 0x3C
    assert np.bincount(subs_of(recs) & 511).max() <= 1024
    assert len(np.unique(prefixes(recs))) == n
    got, fused = both(nat, recs)
    assert fused == 1
    assert np.array_equal(got, oracle.sort_records(recs))


# ---- 3. equal prefixes --------------------------------------------------

def plant_run(recs, rows, tails):
    """rows[1:] get the prefix of rows[0]; byte 8 of each row = tails"""
    recs[rows[1:], :8] = recs[rows[0], :8]
    recs[rows, 8] = tails


def plant_neighbour(recs, row, home, low_byte=7):
    """row gets home's prefix with its lowest bit flipped: another key in
    the same sub-bucket, so that sub-bucket is sorted and does not take the
    all-equal shortcut"""
    recs[row, :8] = recs[home, :8]
    recs[row, low_byte] ^= 0x01


@pytest.mark.parametrize("where", ["first", "last", "eight"])
def test_short_tie_settled_in_block(nat, oracle, where):
    n = 1 << 17
    recs = uniform(oracle, n)[0].copy()
    sub = subs_of(recs)
    by_sub = np.argsort(sub, kind="stable")
    if where == "first":
        homes = [by_sub[0]]
    elif where == "last":
        homes = [by_sub[-1]]
    else:
        homes = [by_sub[(2 * k + 1) * n // 16] for k in range(8)]
    free = iter(np.setdiff1d(np.arange(n), homes)[::997])
    for h in homes:
        o = next(free)
        i, j = min(h, o), max(h, o)
        if i != h:
            recs[i, :8] = recs[h, :8]
        # the stable pair sort leaves (i, j); the full-record order is
        # (j, i)
        plant_run(recs, np.array([i, j]), [0xFF, 0x00])
        # a third record with another key in the same sub-bucket, so that
        # this is a tie inside a sorted sub-bucket and not the all-equal
        # shortcut
        plant_neighbour(recs, next(free), h)
    assert n - len(np.unique(prefixes(recs))) == len(homes)
    got, fused = both(nat, recs)
    assert fused == 1
    assert np.array_equal(got, oracle.sort_records(recs))
    assert_fully_ordered(got)


@pytest.mark.parametrize("length,want", [(8, 1), (9, 2)])
def test_run_length_limit(nat, oracle, length, want):
    # distinct tails, descending in input order; 8 is the longest run the
    # block settles
    n = 1 << 17
    recs = uniform(oracle, n)[0].copy()
    rows = np.arange(length) * 4099 + 17
    plant_run(recs, rows, 200 - np.arange(length))
    plant_neighbour(recs, 3, rows[0])
    got, fused = both(nat, recs)
    assert fused == want
    assert np.array_equal(got, oracle.sort_records(recs))
    assert_fully_ordered(got)


def test_all_equal_sub_bucket(nat, oracle):
    # 600 identical records alone in one sub-bucket: the all-equal shortcut
    n = 1 << 17
    recs = uniform(oracle, n)[0].copy()
    recs[:600] = recs[0]
    sub = subs_of(recs)
    stray = np.flatnonzero(sub[600:] == sub[0]) + 600
    recs[stray, 0] ^= 0x80
    assert np.count_nonzero(subs_of(recs) == sub[0]) == 600
    got, fused = both(nat, recs)
    assert fused == 2
    assert np.array_equal(got, oracle.sort_records(recs))


def test_true_duplicates_run_of_three(nat, oracle):
    n = 1 << 17
    recs = uniform(oracle, n)[0].copy()
    recs[[5000, 70000]] = recs[31]
    plant_neighbour(recs, 3, 31)
    got, fused = both(nat, recs)
    assert fused == 1
    assert np.array_equal(got, oracle.sort_records(recs))
    assert_fully_ordered(got)


# ---- 4. inputs and settings that must take the separate kernels -------

def test_fallback_128_byte_records(nat, oracle):
    n = 1 << 15
    rng = np.random.default_rng(31)
    recs = rng.integers(0, 256, (n, 128)).astype(np.uint8)
    got, fused = both(nat, recs)
    assert fused == 0
    assert np.array_equal(got, oracle.sort_records(recs))


@pytest.mark.parametrize("var,val", [("T9_PASS2_BITS", "8"),
                                     ("T9_MSB_LEVELS", "3"),
                                     ("T9_GATHER_VARIANT", "1")])
def test_fallback_other_flows(nat, oracle, var, val):
    recs, exp = uniform(oracle, (1 << 17) + 3)
    os.environ[var] = val
    got, fused = both(nat, recs)
    assert fused == 0
    assert np.array_equal(got, exp)


def test_fallback_perf_timing(nat, oracle):
    recs, exp = uniform(oracle, (1 << 17) + 3)
    nat.perf_reset()
    nat.perf_enable(True)
    try:
        got, fused = gpu_sort(nat, recs)
        torch.cuda.synchronize()
        _, launches = nat.perf_read("gather")
    finally:
        nat.perf_enable(False)
        nat.perf_reset()
    assert fused == 0
    assert launches == 1
    assert np.array_equal(got, exp)


def test_fallback_chunked_schedule_keeps_precedence(nat, oracle):
    recs, exp = uniform(oracle, (1 << 17) + 3)
    os.environ["T9_SORT_OVERLAP"] = "1"
    got, fused = both(nat, recs)
    assert fused == 0
    assert nat.sort_last_schedule() == 8
    assert np.array_equal(got, exp)


def test_fused_is_the_default(nat, oracle):
    recs, exp = uniform(oracle, (1 << 17) + 3)
    del os.environ["T9_SORT_FUSED_GATHER"]
    got, fused = gpu_sort(nat, recs)
    assert fused == 1
    assert np.array_equal(got, exp)


def test_fused_reports_schedule_zero(nat, oracle):
    recs, exp = uniform(oracle, (1 << 17) + 3)
    got, fused = gpu_sort(nat, recs)
    assert fused == 1 and nat.sort_last_schedule() == 0
    assert np.array_equal(got, exp)


# ---- 5. little-endian key ----------------------------------------------

def test_keyle_100_byte(nat):
    n = (1 << 15) + 5
    rng = np.random.default_rng(41)
    recs = rng.integers(0, 256, (n, 100)).astype(np.uint8)
    # one settled tie: equal keys, tails against the input order
    recs[900, :8] = recs[20, :8]
    recs[20, 8], recs[900, 8] = 0xFF, 0x00
    plant_neighbour(recs, 3, 20, low_byte=0)
    got, fused = both(nat, recs, keyle=True)
    assert fused == 1
    keys = recs[:, :8].copy().view("<u8").reshape(-1)
    order = np.lexsort(tuple(recs[:, c] for c in range(99, 7, -1))
                       + (keys,))
    assert np.array_equal(got, recs[order])


# ---- 6. one context, three sorts, two streams, then close -------------

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
                got, fused = gpu_sort(nat, recs)
            else:
                torch.cuda.synchronize()
                with torch.cuda.stream(st):
                    got, fused = gpu_sort(nat, recs)
                st.synchronize()
            assert fused == 1
            assert np.array_equal(got, oracle.sort_records(recs))
    finally:
        nat.close()
