"""Boundary-shape parity of the reduce support kernels — hash_bucket,
bucket_mod, hash2_of, index_bucket, reduce_by_index — against the numpy
references of tests/_np_ref.py, over the whole output and per bucket, and
the index0 contract of the three generators. Every comparison is exact
equality; buffers are guarded as in test_gpu_sort_support_edges.py."""
import numpy as np
import pytest
import torch

from tests import _np_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tests import _guard as U

ONES = 0xFFFFFFFFFFFFFFFF
FULL = R.GRID_FOR_CAP * 256               # items per trip of the full grid
SIZES = [1, 257, FULL, FULL + 1]
PS = [1, 3, 255, 256]
EDGE_KEYS = np.array([0, 1 << 63, ONES, (1 << 63) - 1, 1, ONES - 1,
                      1 << 32, (1 << 63) + 255], np.uint64)


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


@pytest.fixture(scope="module")
def stream_keys():
    """one fixed stream over the full u64 range; the edge keys come first,
    so every size above 8 holds 0, 2^63 and 2^64-1. Read-only."""
    rng = np.random.default_rng(0xED6E)
    k = rng.integers(0, 1 << 64, FULL + 1, dtype=np.uint64)
    k[:len(EDGE_KEYS)] = EDGE_KEYS
    k.setflags(write=False)
    return k


def key_sets(stream_keys):
    """the inputs of the size ladder; at n = 1 each edge key in turn."""
    for n in SIZES:
        if n == 1:
            for k in EDGE_KEYS[:3]:
                yield np.array([k], np.uint64)
        else:
            yield stream_keys[:n]


def check_buckets(call, keys, p, exp):
    """run call(d_keys, n, d_bucket, d_counts) twice on one counts buffer
    that starts as garbage; whole bucket array and per-bucket counts."""
    n = len(keys)
    cnt = np.bincount(exp, minlength=p).astype(np.uint64)
    dk = U.In(keys)
    dc = U.garbage(p + U.NCAN, np.uint64)
    for _ in range(2):
        db = U.Out(n, np.uint32)
        call(dk.ptr, n, db.ptr, dc.data_ptr())
        U.sync()
        assert np.array_equal(db.read(), exp), (n, p)
        c = U.G.host(dc, np.uint64)
        assert np.array_equal(c[:p], cnt), (n, p)
        assert np.all(c[p:] == U.CANARY[np.uint64]), (n, p)
    dk.check()


@pytest.mark.parametrize("salt", [0, 1, ONES])
@pytest.mark.parametrize("p", PS)
def test_hash_bucket_whole_array_and_counts(nat, stream, stream_keys, p,
                                            salt):
    for keys in key_sets(stream_keys):
        check_buckets(
            lambda k, n, b, c: nat.hash_bucket(k, n, salt, p, b, c, stream),
            keys, p, R.hash_bucket(keys, salt, p))


@pytest.mark.parametrize("p", PS)
def test_bucket_mod_is_an_unsigned_modulo(nat, stream, stream_keys, p):
    for keys in key_sets(stream_keys):
        check_buckets(
            lambda k, n, b, c: nat.bucket_mod(k, n, p, b, c, stream),
            keys, p, R.bucket_mod(keys, p))


def test_hash2_of_values(nat, stream, stream_keys):
    for ids in key_sets(stream_keys):
        n = len(ids)
        e1, e2 = R.hash2_of(ids)
        di = U.In(ids)
        d1, d2 = U.Out(n, np.uint64), U.Out(n, np.uint64)
        nat.hash2_of(di.ptr, n, d1.ptr, d2.ptr, stream)
        U.sync()
        g1, g2 = d1.read(), d2.read()
        assert np.array_equal(g1, e1) and np.array_equal(g2, e2), n
        assert not np.any(g1 == np.uint64(ONES))
        assert not np.any(g2 == np.uint64(ONES))
        di.check()


# ----------------------------------------------------------- index_bucket

@pytest.mark.parametrize("begin,size", [(0, 1), (50, 3), (50, 1024),
                                        (7, 1000)])
@pytest.mark.parametrize("p", PS)
def test_index_bucket_ranges_clamp_and_flag(nat, stream, p, begin, size):
    rng = np.random.default_rng(p * 1031 + size)
    lo, hi = begin, begin + size - 1
    # keys outside [begin, begin+size): below (if there is room), just
    # above, and far above
    outside = ([begin - 1, 0] if begin else []) + [hi + 1, ONES, 1 << 63]
    for n in SIZES:
        keys = rng.integers(lo, hi + 1, n).astype(np.uint64)
        keys[0] = lo
        keys[-1] = hi if n > 1 else keys[-1]
        cases = [(keys, 0)]
        if n == 1:
            cases.append((np.array([hi], np.uint64), 0))
            cases += [(np.array([k], np.uint64), 1) for k in outside]
        else:
            bad = keys.copy()
            at = np.linspace(1, n - 2, len(outside)).astype(int)
            bad[at] = np.array(outside, np.uint64)
            cases.append((bad, 1))
        for ks, flag in cases:
            exp, eflag = R.index_bucket(ks, begin, size, p)
            assert eflag == flag
            if flag:
                last = int(exp[np.isin(ks, np.array(outside, np.uint64))][0])
                assert last == (size - 1) * p // size
            de = U.garbage(1 + U.NCAN, np.uint32)
            check_buckets(
                lambda k, m, b, c: nat.index_bucket(
                    k, m, begin, size, p, b, c, de.data_ptr(), stream),
                ks, p, exp)
            e = U.G.host(de, np.uint32)
            assert int(e[0]) == flag, (n, flag)
            assert np.all(e[1:] == U.CANARY[np.uint32])


# -------------------------------------------------------- reduce_by_index

def run_reduce_by_index(nat, stream, keys, vals, begin, size):
    n = len(keys)
    dk, dv = U.In(keys), U.In(vals)
    dd = U.Out(size, np.uint64)           # the payload starts as garbage
    de = U.garbage(1 + U.NCAN, np.uint32)
    nat.reduce_by_index(dk.ptr, dv.ptr, n, begin, size, dd.ptr,
                        de.data_ptr(), stream)
    U.sync()
    e = U.G.host(de, np.uint32)
    assert np.all(e[1:] == U.CANARY[np.uint32])
    dk.check()
    dv.check()
    return dd.read(), int(e[0])


@pytest.mark.parametrize("size", [1, 2, 5000])
@pytest.mark.parametrize("n", [1, 257, FULL + 1])
def test_reduce_by_index_one_cell_takes_everything(nat, stream, n, size):
    # maximal contention on one cell, and the sum wraps 2^64 many times
    rng = np.random.default_rng(n + size)
    begin = 1000
    keys = np.full(n, begin + size // 2, np.uint64)
    vals = np.uint64(1 << 63) + rng.integers(0, 1 << 20, n).astype(np.uint64)
    exp, flag = R.reduce_by_index(keys, vals, begin, size)
    assert flag == 0 and np.count_nonzero(exp) <= 1
    got, gflag = run_reduce_by_index(nat, stream, keys, vals, begin, size)
    assert gflag == 0
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("size", [1, 2, 5000])
@pytest.mark.parametrize("n", [1, 257, FULL + 1])
def test_reduce_by_index_out_of_range_on_both_sides(nat, stream, n, size):
    # keys below begin and behind the range among valid ones: the flag is
    # set, the valid ones are still summed, untouched cells read zero
    rng = np.random.default_rng(n * 3 + size)
    begin = 1000
    used = max(1, size // 2)              # cells behind `used` stay empty
    keys = rng.integers(begin, begin + used, n).astype(np.uint64)
    vals = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    outside = np.array([begin - 1, 0, begin + size, ONES, 1 << 63],
                       np.uint64)
    if n == 1:
        keys[0] = outside[0]
    else:
        keys[np.linspace(0, n - 1, len(outside)).astype(int)] = outside
    exp, flag = R.reduce_by_index(keys, vals, begin, size)
    assert flag == 1
    got, gflag = run_reduce_by_index(nat, stream, keys, vals, begin, size)
    assert gflag == 1
    assert np.array_equal(got, exp)
    if size > 1:
        assert not np.any(got[used:])


# ------------------------------------------------------------- generators

K0, GN = 1000, 4097


def test_gen_u64_index0_is_an_offset_into_one_stream(nat, oracle, stream):
    whole, part = U.Out(GN + K0, np.uint64), U.Out(GN, np.uint64)
    nat.gen_u64(whole.ptr, 0, GN + K0, 0x5EED, stream)
    nat.gen_u64(part.ptr, K0, GN, 0x5EED, stream)
    U.sync()
    w, p = whole.read(), part.read()
    assert np.array_equal(p, w[K0:])
    assert np.array_equal(w, oracle.gen_u64(GN + K0, seed=0x5EED))
    assert np.array_equal(p, oracle.gen_u64(GN, seed=0x5EED, index0=K0))


def test_gen_records_index0_is_an_offset_into_one_stream(nat, oracle,
                                                         stream):
    whole = U.Out((GN + K0) * 100, np.uint8)
    part = U.Out(GN * 100, np.uint8)
    nat.gen_records(whole.ptr, 0, GN + K0, 0x5EED, stream)
    nat.gen_records(part.ptr, K0, GN, 0x5EED, stream)
    U.sync()
    w = whole.read().reshape(GN + K0, 100)
    p = part.read().reshape(GN, 100)
    assert np.array_equal(p, w[K0:])
    assert np.array_equal(w, oracle.gen_records(GN + K0, seed=0x5EED))
    assert np.array_equal(p, oracle.gen_records(GN, seed=0x5EED, index0=K0))


def test_zipf_tokens_index0_is_an_offset_into_one_stream(nat, oracle,
                                                         stream):
    vocab = 1000
    cdf = oracle.zipf_cdf(vocab, 1.1)
    dcdf = U.In(cdf)
    whole, part = U.Out(GN + K0, np.uint64), U.Out(GN, np.uint64)
    nat.zipf_tokens(whole.ptr, dcdf.ptr, vocab, 0, GN + K0, 9, stream)
    nat.zipf_tokens(part.ptr, dcdf.ptr, vocab, K0, GN, 9, stream)
    U.sync()
    w, p = whole.read(), part.read()
    assert np.array_equal(p, w[K0:])
    assert np.array_equal(w, oracle.zipf_tokens(cdf, GN + K0, seed=9))
    assert np.array_equal(p, oracle.zipf_tokens(cdf, GN, seed=9, index0=K0))
    dcdf.check()
