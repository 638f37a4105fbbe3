"""GPU tests of the packed record sort (k_scatter_seg9_packed +
k_wave16_sort_gather_packed): where the fused sort + gather kernel runs and
n <= 2^27, pass 2 emits one u64 per element, (key bits 46..10) << 27 |
record index, and the fused kernel sorts those as they are. Key bits 9..0
are dropped, so neighbours that agree in the kept bits are candidate ties,
true (equal 8-byte keys) or false (keys that differ in the dropped bits);
runs of up to 8 are settled in the block by the full record order, longer
ones make the wide form redo pass 2 and the sort.

Every case is compared byte for byte against the CPU order AND against the
same call with T9_SORT_PACKED=0, asserts through t9_sort_last_packed which
path ran (1 = packed produced the output, 2 = it started and the wide form
redid it, 0 = not used), that the input is unchanged and that the sentinel
guards round d_out are intact.

Sub-bucket of a record = top 17 bits of its key (256 x 512 sub-buckets);
at n <= 2^17 most of them hold 0, 1 or 2 records."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tests import _gpu as G
    from thrill_amd import Native

GUARD = 4096
SENTINEL = 0xA5
KNOBS = ("T9_SORT_ALGO", "T9_SORT_FUSED_GATHER", "T9_SORT_OVERLAP",
         "T9_SORT_OVERLAP_CHUNKS", "T9_PASS2_BITS", "T9_MSB_LEVELS",
         "T9_GATHER_VARIANT", "T9_EXTRACT_IOTA", "T9_SORT_PACKED",
         "T9_SORT_PACKED_IDXBITS")


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = Native(device=0)
    yield n
    n.close()


@pytest.fixture(autouse=True)
def packed_env():
    saved = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ["T9_SORT_ALGO"] = "msb"
    os.environ["T9_SORT_PACKED"] = "1"
    yield
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def keys_of(recs, keyle=False):
    return recs[:, :8].copy().view("<u8" if keyle else ">u8").reshape(-1)


def subs_of(recs, keyle=False):
    return (keys_of(recs, keyle) >> np.uint64(47)).astype(np.int64)


def set_key(recs, row, key, keyle=False):
    recs[row, :8] = np.array([key], dtype="<u8" if keyle else ">u8").view(
        np.uint8)


def cpu_sorted(oracle, recs, keyle=False):
    """the full order: the 64-bit key as the entry defines it, then bytes
    8..99. Big-endian keys: that is the oracle's bytewise order."""
    if not keyle:
        return oracle.sort_records(recs)
    order = np.lexsort(tuple(recs[:, c] for c in range(99, 7, -1))
                       + (keys_of(recs, keyle),))
    return recs[order]


def gpu_sort(nat, recs, keyle=False):
    """-> (output, last_packed, last_fused); d_out sits between two
    sentinel guards and both are checked"""
    n, rs = recs.shape
    din = G.dev(recs.reshape(-1))
    buf = torch.full((n * rs + 2 * GUARD,), SENTINEL, dtype=torch.uint8,
                     device="cuda")
    dout = buf[GUARD:GUARD + n * rs]
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
    h = G.host(buf, np.uint8)
    assert (h[:GUARD] == SENTINEL).all(), "front guard overwritten"
    assert (h[GUARD + n * rs:] == SENTINEL).all(), "back guard overwritten"
    return got, nat.sort_last_packed(), nat.sort_last_fused()


def both(nat, recs, keyle=False):
    """(output, packed, fused) of the run as the environment stands; the
    T9_SORT_PACKED=0 run must not pack and be byte-identical"""
    got, packed, fused = gpu_sort(nat, recs, keyle)
    os.environ["T9_SORT_PACKED"] = "0"
    try:
        wide, p0, f0 = gpu_sort(nat, recs, keyle)
    finally:
        os.environ["T9_SORT_PACKED"] = "1"
    assert p0 == 0
    assert np.array_equal(got, wide), "packed != wide"
    if packed == 2:
        # the redo is a wide run: it reports what the wide run reports
        assert fused == f0
    return got, packed, fused


_uniform = {}


def uniform(oracle, n):
    """seeded uniform records and their order, computed once (tests that
    plant records work on a copy). No two keys agree in bits 63..10."""
    if n not in _uniform:
        recs = oracle.gen_records(n, seed=0x9AC + n)
        assert len(np.unique(keys_of(recs) >> np.uint64(10))) == n
        exp = oracle.sort_records(recs)
        exp.setflags(write=False)
        _uniform[n] = (recs, exp)
    return _uniform[n]


N17 = (1 << 17) + 3


def crowd(recs, home, rows, keyle=False):
    """rows get home's key with one of bits 10..12 changed: other
    composites in home's sub-bucket, so that the candidates planted there
    are runs inside a sorted sub-bucket"""
    k = int(keys_of(recs[home:home + 1], keyle)[0])
    for t, r in enumerate(rows):
        set_key(recs, r, k ^ (1 << (10 + t)), keyle)


def plant_low(recs, rows, lows, keyle=False, tails=None):
    """rows get the key of rows[0] with bits 9..0 = lows; byte 8 = tails"""
    k = int(keys_of(recs[rows[0]:rows[0] + 1], keyle)[0]) & ~0x3FF
    for r, lo in zip(rows, lows):
        set_key(recs, r, k | int(lo), keyle)
    if tails is not None:
        recs[rows, 8] = tails


# ---- 1. uniform --------------------------------------------------------

@pytest.mark.parametrize("n", [1 << 14, (1 << 14) + 1, N17])
def test_uniform(nat, oracle, n):
    recs, exp = uniform(oracle, n)
    got, packed, fused = both(nat, recs)
    assert packed == 1 and fused == 1
    assert np.array_equal(got, exp)


def test_dense_sub_buckets(nat, oracle):
    # 2^17 records over 160 sub-buckets: about 819 each, at most 1024
    n = 1 << 17
    recs = oracle.gen_records(n, seed=0xD5).copy()
    recs[:, 0] = 0x3C
    recs[:, 1] = np.arange(n) % 80
    cnt = np.bincount(subs_of(recs) & 511)
    assert np.count_nonzero(cnt) == 160
    assert 700 <= cnt.max() <= 1024
    assert len(np.unique(keys_of(recs) >> np.uint64(10))) == n
    got, packed, fused = both(nat, recs)
    assert packed == 1 and fused == 1
    assert np.array_equal(got, oracle.sort_records(recs))


def test_packed_is_the_default(nat, oracle):
    recs, exp = uniform(oracle, N17)
    del os.environ["T9_SORT_PACKED"]
    got, packed, fused = gpu_sort(nat, recs)
    os.environ["T9_SORT_PACKED"] = "1"
    assert packed == 1 and fused == 1
    assert np.array_equal(got, exp)


# ---- 2. false ties: keys that differ in the dropped bits only ------------

@pytest.mark.parametrize("keyle", [False, True])
@pytest.mark.parametrize("order", ["sorted", "reversed"])
@pytest.mark.parametrize("crowded", [False, True])
def test_false_tie_run_of_two(nat, oracle, keyle, order, crowded):
    # big-endian: the dropped bits are byte 7 and two bits of byte 6;
    # keyle: byte 0 and two bits of byte 1. The tails point the other way,
    # so the order must come from the key.
    recs = uniform(oracle, N17)[0].copy()
    i, j = 1234, 98765
    lows = [0x005, 0x2F0] if order == "sorted" else [0x2F0, 0x005]
    tails = [0xFF, 0x00] if order == "sorted" else [0x00, 0xFF]
    plant_low(recs, [i, j], lows, keyle, tails)
    if crowded:
        crowd(recs, i, [77, 50001], keyle)
    got, packed, fused = both(nat, recs, keyle)
    assert packed == 1 and fused == 1
    assert np.array_equal(got, cpu_sorted(oracle, recs, keyle))


@pytest.mark.parametrize("keyle", [False, True])
def test_false_tie_run_of_eight(nat, oracle, keyle):
    recs = uniform(oracle, N17)[0].copy()
    rows = list(np.arange(8) * 4099 + 17)
    lows = [0x3FF, 0x000, 0x100, 0x0FF, 0x200, 0x001, 0x2AA, 0x155]
    plant_low(recs, rows, lows, keyle, tails=np.arange(8))
    crowd(recs, rows[0], [3, 60000], keyle)
    got, packed, fused = both(nat, recs, keyle)
    assert packed == 1 and fused == 1
    assert np.array_equal(got, cpu_sorted(oracle, recs, keyle))


# ---- 3. real ties --------------------------------------------------------

@pytest.mark.parametrize("keyle", [False, True])
def test_real_tie_tails_against_input_order(nat, oracle, keyle):
    recs = uniform(oracle, N17)[0].copy()
    i, j = 4321, 87654
    plant_low(recs, [i, j], [0x123, 0x123], keyle, tails=[0xFF, 0x00])
    crowd(recs, i, [9], keyle)
    got, packed, fused = both(nat, recs, keyle)
    assert packed == 1 and fused == 1
    assert np.array_equal(got, cpu_sorted(oracle, recs, keyle))


def test_true_duplicates(nat, oracle):
    # identical records: any order of them is the same bytes, so what is
    # checked is that each appears as often as it was planted and that the
    # rest of the output is untouched by them
    recs = uniform(oracle, N17)[0].copy()
    recs[[5000, 70000]] = recs[31]
    crowd(recs, 31, [3])
    got, packed, fused = both(nat, recs)
    assert packed == 1 and fused == 1
    exp = cpu_sorted(oracle, recs)
    assert np.array_equal(got, exp)
    assert np.count_nonzero((got == recs[31]).all(axis=1)) == 3


@pytest.mark.parametrize("keyle", [False, True])
def test_run_mixing_real_and_false_ties(nat, oracle, keyle):
    # 7 candidates: two pairs of equal keys with different tails, one pair
    # of identical records, one key of its own
    recs = uniform(oracle, N17)[0].copy()
    rows = [100, 20100, 40100, 60100, 80100, 100100, 120100]
    lows = [0x300, 0x010, 0x300, 0x010, 0x1FF, 0x1FF, 0x000]
    plant_low(recs, rows, lows, keyle, tails=[9, 8, 7, 6, 5, 5, 4])
    recs[rows[5]] = recs[rows[4]]
    got, packed, fused = both(nat, recs, keyle)
    assert packed == 1 and fused == 1
    assert np.array_equal(got, cpu_sorted(oracle, recs, keyle))


# ---- 4. what the block cannot settle ------------------------------------

@pytest.mark.parametrize("keyle", [False, True])
def test_long_run_of_false_ties(nat, oracle, keyle):
    # 9 candidates with 9 different keys: the packed run gives up, the
    # wide run meets no tie at all
    recs = uniform(oracle, N17)[0].copy()
    rows = list(np.arange(9) * 4099 + 17)
    plant_low(recs, rows, 0x3FF - 100 * np.arange(9), keyle)
    crowd(recs, rows[0], [3], keyle)
    got, packed, fused = both(nat, recs, keyle)
    assert packed == 2 and fused == 1
    assert nat.sort_last_tiecount() == 1
    assert np.array_equal(got, cpu_sorted(oracle, recs, keyle))


def test_long_run_of_real_ties(nat, oracle):
    # 9 equal keys: too long for the wide kernel's block as well
    recs = uniform(oracle, N17)[0].copy()
    rows = list(np.arange(9) * 4099 + 17)
    plant_low(recs, rows, [0x155] * 9, tails=200 - np.arange(9))
    crowd(recs, rows[0], [3])
    got, packed, fused = both(nat, recs)
    assert packed == 2 and fused == 2
    assert np.array_equal(got, cpu_sorted(oracle, recs))


def test_all_equal_sub_bucket_false_ties(nat, oracle):
    # 600 records alone in one sub-bucket, equal in bits 63..10 and all
    # different below
    recs = uniform(oracle, N17)[0].copy()
    m = 600
    rng = np.random.default_rng(5)
    plant_low(recs, list(range(m)), rng.permutation(1024)[:m])
    sub = subs_of(recs)
    stray = np.flatnonzero(sub[m:] == sub[0]) + m
    recs[stray, 0] ^= 0x80
    assert np.count_nonzero(subs_of(recs) == sub[0]) == m
    got, packed, fused = both(nat, recs)
    assert packed == 2 and fused == 1
    assert np.array_equal(got, cpu_sorted(oracle, recs))


def test_all_equal_sub_bucket_identical(nat, oracle):
    recs = uniform(oracle, N17)[0].copy()
    m = 600
    recs[:m] = recs[0]
    sub = subs_of(recs)
    stray = np.flatnonzero(sub[m:] == sub[0]) + m
    recs[stray, 0] ^= 0x80
    got, packed, fused = both(nat, recs)
    assert packed == 2 and fused == 2
    assert np.array_equal(got, cpu_sorted(oracle, recs))


# ---- 5. where packed mode is refused -------------------------------------

@pytest.mark.parametrize("bits,n,want", [(16, 1 << 17, 0), (17, 1 << 17, 1),
                                         (17, (1 << 17) + 3, 0)])
def test_index_bound_hook(nat, oracle, bits, n, want):
    recs, exp = uniform(oracle, n)
    os.environ["T9_SORT_PACKED_IDXBITS"] = str(bits)
    got, packed, fused = both(nat, recs)
    assert packed == want and fused == 1
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("m", [1025, 5000])
def test_ineligible_sub_bucket(nat, oracle, m):
    # one sub-bucket above the 1024 tier, and one above every LDS tier
    recs = uniform(oracle, N17)[0].copy()
    recs[:m, 0] = 0x5A
    recs[:m, 1] = 0xC3
    recs[:m, 2] &= 0x7F
    assert np.count_nonzero(subs_of(recs) == subs_of(recs)[0]) >= m
    got, packed, fused = both(nat, recs)
    assert packed == 0 and fused == 0
    assert np.array_equal(got, oracle.sort_records(recs))


def test_fused_off_means_not_packed(nat, oracle):
    recs, exp = uniform(oracle, N17)
    os.environ["T9_SORT_FUSED_GATHER"] = "0"
    got, packed, fused = both(nat, recs)
    assert packed == 0 and fused == 0
    assert np.array_equal(got, exp)
