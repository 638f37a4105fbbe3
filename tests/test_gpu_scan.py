"""GPU tests of the scan family (t9_scan_u64 / t9_scan_kv / t9_fold_u64 and
pipeline.PrefixSum) against numpy (tests/_scan_ref.py). Every comparison
is exact equality of 64-bit patterns. Sizes come from t9_scan_geometry:
with T the tile and P the tile totals per block of the middle pass, the
ladder crosses every wave, round, tile and pass-2 level boundary.

Every call runs on a workspace pre-filled with 0xFF bytes, writes into a
buffer with 64 canary elements behind it, and leaves its input alone."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _scan_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tests import _gpu as G

CANARY = np.uint64(0xC0FFEE00DEADBEEF)
NCAN = 64
IDS = {(op, vt): "%s-%s" % (("sum", "min", "max")[op],
                            ("u64", "i64", "f64")[vt])
       for op, vt in R.VALID}
VALID_IDS = [IDS[c] for c in R.VALID]


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from thrill_amd import Native
    n = Native(device=0)
    yield n
    n.close()


@pytest.fixture(scope="module")
def geo(nat):
    T, P = nat.scan_geometry()
    sizes = [0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, T - 1, T,
             T + 1, 2 * T + 3, P * T + 5, (P + 1) * T + T // 2]
    return T, P, sizes


@functools.lru_cache(maxsize=None)
def data(vt, n):
    """the first n of one fixed random stream per value type (so the sizes
    of the ladder are prefixes of each other); read-only."""
    x = R.values(n, vt, seed=0xD1A0 + vt)
    x.setflags(write=False)
    return x


def initial_of(vt):
    return {R.U64: 0x9E3779B97F4A7C15, R.I64: 0xFFFFFFFFFFFF0001,
            R.F64: 0x4059000000000000}[vt]


def filled_ws(nat, n):
    w = G.ws(nat.ws("scan", n))
    w.fill_(0xFF)
    return w


def scan_u64(nat, x, op, vt, ex, init, in_place=False, w=None, offset=0):
    """run t9_scan_u64 on x; returns (out, total) after checking the
    canaries and that the input is unchanged. offset shifts input and
    output by that many u64 words inside their allocations."""
    n = len(x)
    buf = np.concatenate([np.zeros(offset, np.uint64), x,
                          np.full(NCAN, CANARY)])
    d_in = G.dev(buf)
    d_out = d_in if in_place else G.dev(
        np.full(offset + n + NCAN, CANARY, np.uint64))
    d_tot = G.dev(np.array([CANARY], np.uint64))
    w = filled_ws(nat, n) if w is None else w
    pin = d_in.data_ptr() + 8 * offset
    pout = d_out.data_ptr() + 8 * offset
    nat.scan_u64(pin if n else None, pout if n else None, n, op, vt, ex,
                 init, G.ptr(d_tot), G.ptr(w), G.stream())
    torch.cuda.synchronize()
    out = G.host(d_out, np.uint64)
    assert np.all(out[offset + n:] == CANARY), "wrote past d_out[n-1]"
    if not in_place:
        assert np.all(out[:offset] == CANARY), "wrote before d_out[0]"
        assert np.array_equal(G.host(d_in, np.uint64), buf), \
            "d_in changed"
    return out[offset:offset + n], int(G.host(d_tot, np.uint64)[0])


@pytest.mark.parametrize("op,vt", R.VALID, ids=VALID_IDS)
def test_scan_size_ladder(nat, geo, op, vt):
    T, P, sizes = geo
    init = initial_of(vt)
    for n in sizes:
        x = data(vt, sizes[-1])[:n]
        for ex in (0, 1):
            out, tot = scan_u64(nat, x, op, vt, ex, init)
            assert np.array_equal(out, R.scan(x, op, vt, ex, init)), \
                (n, ex)
            assert tot == R.fold(x, op, vt), (n, ex)


@pytest.mark.parametrize("vt", [R.U64, R.I64, R.F64])
def test_min_over_strictly_decreasing(nat, geo, vt):
    """every element lowers the minimum, in the value type's own order."""
    T, P, _ = geo
    n = 2 * T + 3
    e = np.uint64(1 << 63) + np.arange(n, 0, -1, dtype=np.uint64) * \
        np.uint64(0x0000100000000001)
    x = R.dec(e, R.MIN, vt)
    top = R.identity(R.MIN, vt)
    out, tot = scan_u64(nat, x, R.MIN, vt, 0, top)
    assert np.array_equal(out, x)
    assert tot == int(x[-1])
    out, _ = scan_u64(nat, x, R.MIN, vt, 1, top)
    assert np.array_equal(out[1:], x[:-1]) and int(out[0]) == top


@pytest.mark.parametrize("vt", [R.U64, R.I64, R.F64])
@pytest.mark.parametrize("where", ["T-1", "T"])
def test_max_single_extreme_carries_over_the_tile_edge(nat, geo, vt, where):
    T, P, _ = geo
    n, at = 2 * T + 3, (T - 1 if where == "T-1" else T)
    zero, big = 0, int(R.dec(np.array([R.ONES - np.uint64(7)]), R.MAX,
                             vt)[0])
    x = np.full(n, zero, np.uint64)
    x[at] = big
    bottom = R.identity(R.MAX, vt)
    for ex in (0, 1):
        out, tot = scan_u64(nat, x, R.MAX, vt, ex, bottom)
        assert np.array_equal(out, R.scan(x, R.MAX, vt, ex, bottom))
        first = at + ex
        assert np.all(out[first:] == np.uint64(big))
        assert not np.any(out[:first] == np.uint64(big))
        assert tot == big


@pytest.mark.parametrize("op,vt", R.VALID, ids=VALID_IDS)
def test_initial_zero_nonzero_dominating(nat, geo, op, vt):
    T, P, _ = geo
    x = data(vt, geo[2][-1])[:T + 1]
    inits = [0, initial_of(vt)]
    if op != R.SUM:
        # MAX seeded with the top of the order (all-ones for U64), MIN with
        # the bottom: the initial value is every output
        dom = R.identity(R.MIN if op == R.MAX else R.MAX, vt)
        inits.append(dom)
    for init in inits:
        for ex in (0, 1):
            out, tot = scan_u64(nat, x, op, vt, ex, init)
            assert np.array_equal(out, R.scan(x, op, vt, ex, init))
            assert tot == R.fold(x, op, vt)      # never includes initial
    if op != R.SUM:
        assert np.all(out == np.uint64(dom))
    if op == R.MAX and vt == R.U64:
        assert dom == (1 << 64) - 1


@pytest.mark.parametrize("op,vt", R.VALID, ids=VALID_IDS)
def test_fold_stride_1_and_2(nat, geo, op, vt):
    T, P, _ = geo
    for n in (1, 2, 257, T - 1, T, T + 1, 2 * T + 3, P * T + 5):
        x = data(vt, geo[2][-1])[:n]
        expect = R.fold(x, op, vt)
        pairs = np.empty(2 * n, np.uint64)
        pairs[0::2] = data(R.U64, geo[2][-1])[:n]    # keys: noise
        pairs[1::2] = x
        for stride, src in ((1, x), (2, pairs)):
            d_in = G.dev(np.array(src))      # the shared data is read-only
            d_res = G.dev(np.array([CANARY], np.uint64))
            nat.fold_u64(G.ptr(d_in), n, stride, op, vt, G.ptr(d_res),
                         G.ptr(filled_ws(nat, n)), G.stream())
            assert int(G.host(d_res, np.uint64)[0]) == expect, (n, stride)
            assert np.array_equal(G.host(d_in, np.uint64), src)


@pytest.mark.parametrize("op,vt", R.VALID, ids=VALID_IDS)
def test_empty_input_gives_the_decoded_identity(nat, op, vt):
    expect = R.identity(op, vt)
    if op == R.MIN:
        assert expect == {R.U64: (1 << 64) - 1, R.I64: (1 << 63) - 1,
                          R.F64: 0x7FFFFFFFFFFFFFFF}[vt]
    if op == R.MAX:
        assert expect == {R.U64: 0, R.I64: 1 << 63,
                          R.F64: 0xFFFFFFFFFFFFFFFF}[vt]
    if op == R.SUM:
        assert expect == 0
    _, tot = scan_u64(nat, np.zeros(0, np.uint64), op, vt, 0, 5)
    assert tot == expect
    d_res = G.dev(np.array([CANARY], np.uint64))
    nat.fold_u64(None, 0, 1, op, vt, G.ptr(d_res), None, G.stream())
    assert int(G.host(d_res, np.uint64)[0]) == expect
    kv_tot = G.dev(np.array([CANARY], np.uint64))
    nat.scan_kv(None, None, 0, op, vt, 5, G.ptr(kv_tot), None, G.stream())
    assert int(G.host(kv_tot, np.uint64)[0]) == expect


def test_two_sizes_back_to_back_on_one_workspace(nat, geo):
    """nothing in the workspace survives a call or is assumed by the
    next: a two-level scan, then a small one, then the big one again."""
    T, P, sizes = geo
    big, small = P * T + 5, 3 * T + 1
    w = filled_ws(nat, big)
    for n in (big, small, big):
        x = data(R.I64, sizes[-1])[:n]
        out, tot = scan_u64(nat, x, R.MIN, R.I64, 1, 17, w=w)
        assert np.array_equal(out, R.scan(x, R.MIN, R.I64, 1, 17)), n
        assert tot == R.fold(x, R.MIN, R.I64)


@pytest.mark.parametrize("op,vt", [(R.SUM, R.U64), (R.MAX, R.F64)],
                         ids=["sum-u64", "max-f64"])
def test_in_place(nat, geo, op, vt):
    T, P, sizes = geo
    for n in (1, 513, T + 1, 2 * T + 3, P * T + 5):
        x = data(vt, sizes[-1])[:n]
        for ex in (0, 1):
            out, _ = scan_u64(nat, x, op, vt, ex, 3, in_place=True)
            assert np.array_equal(out, R.scan(x, op, vt, ex, 3)), (n, ex)


def test_eight_byte_aligned_pointers(nat, geo):
    """d_in / d_out that are 8- but not 16-byte aligned take the narrow
    accesses and give the same result."""
    T, P, sizes = geo
    for n in (1, 2, 513, 2 * T + 3):
        x = data(R.U64, sizes[-1])[:n]
        for ex in (0, 1):
            out, tot = scan_u64(nat, x, R.SUM, R.U64, ex, 9, offset=1)
            assert np.array_equal(out, R.scan(x, R.SUM, R.U64, ex, 9))
            assert tot == R.fold(x, R.SUM, R.U64)


def test_pass1_reverse_order_gives_the_same_result(nat, geo, monkeypatch):
    T, P, sizes = geo
    monkeypatch.setenv("T9_SCAN_P1_REVERSE", "1")
    for n in (1, T + 1, 5 * T + 7, P * T + 5):
        x = data(R.I64, sizes[-1])[:n]
        out, tot = scan_u64(nat, x, R.MAX, R.I64, 0, 1)
        assert np.array_equal(out, R.scan(x, R.MAX, R.I64, 0, 1)), n
        assert tot == R.fold(x, R.MAX, R.I64)


# --------------------------------------------------------------- pairs

def scan_kv(nat, keys, vals, op, vt, init, in_place=False):
    n = len(keys)
    pairs = np.empty(2 * n, np.uint64)
    pairs[0::2], pairs[1::2] = keys, vals
    buf = np.concatenate([pairs, np.full(NCAN, CANARY)])
    d_in = G.dev(buf)
    d_out = d_in if in_place else G.dev(
        np.full(2 * n + NCAN, CANARY, np.uint64))
    d_tot = G.dev(np.array([CANARY], np.uint64))
    nat.scan_kv(G.ptr(d_in) if n else None, G.ptr(d_out) if n else None, n,
                op, vt, init, G.ptr(d_tot), G.ptr(filled_ws(nat, n)),
                G.stream())
    torch.cuda.synchronize()
    out = G.host(d_out, np.uint64)
    assert np.all(out[2 * n:] == CANARY), "wrote past the last pair"
    if not in_place:
        assert np.array_equal(G.host(d_in, np.uint64), buf), "d_in changed"
    return out[0:2 * n:2], out[1:2 * n:2], int(G.host(d_tot, np.uint64)[0])


@pytest.mark.parametrize("op,vt", [(R.SUM, R.U64), (R.MIN, R.U64),
                                   (R.MAX, R.U64), (R.MAX, R.I64)],
                         ids=["sum-u64", "min-u64", "max-u64", "max-i64"])
def test_scan_kv_size_ladder(nat, geo, op, vt):
    T, P, sizes = geo
    init = initial_of(vt)
    for n in sizes:
        keys = data(R.F64, sizes[-1])[:n]      # any patterns at all
        vals = data(vt, sizes[-1])[:n]
        k, v, tot = scan_kv(nat, keys, vals, op, vt, init)
        assert np.array_equal(k, keys), n
        assert np.array_equal(v, R.scan(vals, op, vt, 0, init)), n
        assert tot == R.fold(vals, op, vt), n
    k, v, _ = scan_kv(nat, keys, vals, op, vt, init, in_place=True)
    assert np.array_equal(k, keys)
    assert np.array_equal(v, R.scan(vals, op, vt, 0, init))


def test_scan_kv_names_the_runs_of_prefix_doubling(nat, geo):
    """the prefix-doubling shape: value 0 except at run starts, which hold
    index + 1; a max-scan gives every item the name of its run."""
    T, P, _ = geo
    n = 3 * T + 11
    rng = np.random.default_rng(0x5A5A)
    start = rng.random(n) < 0.01
    start[0] = True
    start[T] = True                      # a run starting on a tile edge
    idx = np.arange(n, dtype=np.uint64)
    vals = np.where(start, idx + np.uint64(1), np.uint64(0))
    keys = rng.permutation(n).astype(np.uint64)
    k, v, tot = scan_kv(nat, keys, vals, R.MAX, R.U64, 0)
    # known answer: the index of the nearest run start at or before i
    name = np.maximum.accumulate(np.where(start, idx, np.uint64(0)))
    assert np.array_equal(v, name + np.uint64(1))
    assert np.array_equal(k, keys)
    assert tot == int(name[-1]) + 1


# ------------------------------------------------------------ pipeline

@pytest.fixture()
def dist_world1():
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    os.environ["T9_FORCE_DIST"] = "1"
    yield dist
    del os.environ["T9_FORCE_DIST"]
    dist.destroy_process_group()


def _pipeline_cases(geo):
    T, P, sizes = geo
    from thrill_amd.pipeline import PrefixSum
    for op, vt, ex in ((R.SUM, R.U64, 0), (R.MIN, R.I64, 1),
                       (R.MAX, R.F64, 0)):
        init = initial_of(vt)
        ps = PrefixSum(op, vt, exclusive=bool(ex), initial=init, rank=0,
                       world=1, device=0)
        for n in (0, 1, 2 * T + 3):
            x = data(vt, sizes[-1])[:n]
            d = G.dev(np.array(x))
            out = ps.step(d)
            assert out.dtype == d.dtype and out.numel() == n
            assert np.array_equal(G.host(out, np.uint64),
                                  R.scan(x, op, vt, ex, init)), (op, vt, n)
            assert ps.reduce(d) == R.fold(x, op, vt), (op, vt, n)
            assert np.array_equal(G.host(d, np.uint64), x)
        ps.close()


def test_pipeline_prefix_sum_world1(nat, geo):
    assert not os.environ.get("T9_FORCE_DIST")
    _pipeline_cases(geo)


def test_pipeline_prefix_sum_distributed_branch_world1(nat, geo,
                                                       dist_world1):
    # T9_FORCE_DIST: fold -> all-gather of the totals -> scan_carry ->
    # scan from the carry, all on one rank
    _pipeline_cases(geo)


def test_pipeline_prefix_sum_refuses_f64_sum():
    from thrill_amd import T9Error
    from thrill_amd.pipeline import PrefixSum
    with pytest.raises(T9Error):
        PrefixSum(R.SUM, R.F64)
