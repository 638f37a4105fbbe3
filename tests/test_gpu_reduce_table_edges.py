"""Edge-shape and variant parity of the reduce hash tables — t9_reduce_
{init,build,drain}, t9_reduce128_{init,build,drain,lookup} and their _op
counterparts — against the numpy references of tests/_np_ref.py.

One harness per table runs init -> build (one or more) -> raw table ->
drain (-> lookup) on guarded buffers: the table sits between canaries,
d_error and d_out_n start as garbage with canaries behind them, drain
outputs are read with valid=m, inputs are compared with their host copy,
and the raw table is read before and after drain. Every comparison is exact
equality, on the drained multiset, on the raw table (one slot per key, an
unbroken probe chain from its home slot) and on the aux sentinel slot.

Every knob-to-kernel mapping of t9_reduce_build (12) and t9_reduce128_build
(6) is a test id; the knobs are read from the environment on every call.

The chain pattern places 12 keys on one LDS slot (SLOTS-2) and one home
slot (14 of 16): 4 fit the 4-probe LDS filter across its wrap, 8 spill to
the global table, whose chain wraps 15 -> 0 next to the aux slot. On the
128-bit table the 12 composites are eight k2 under the first such k1 plus
four more k1 (a 16-slot table cannot hold eight composites for each)."""
import numpy as np
import pytest
import torch

from tests import _np_ref as R
from tests.test_gpu_reduce_ops import (F64, I64, MAX, MIN, SUM, U64, expected,
                                       random_bits)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tests import _guard as U
    from thrill_amd import T9Error

ONES = 0xFFFFFFFFFFFFFFFF
M64 = np.uint64(ONES)
GOLD = np.uint64(0x9E3779B97F4A7C15)
SALTS = [0, 1, ONES]
GRIDS = [None, 1, 3]
NS = [0, 1, 63, 64, 65, 255, 256, 257, 769]
KNOBS = ["T9_REDUCE_COMBINE", "T9_LDS_SLOTS", "T9_REDUCE_READFIRST",
         "T9_REDUCE_WAVECOMB", "T9_LDS128_SLOTS", "T9_R128_READFIRST",
         "T9_R128_STRIDE", "T9_REDUCE_GRID"]


def cfg(slots, **env):
    return {"slots": slots, "env": {k: str(v) for k, v in env.items()}}


# id -> LDS filter slots (None: no filter) and the knobs selecting the kernel
U64_CFGS = {
    "combine0": cfg(None, T9_REDUCE_COMBINE=0),
    "combine1": cfg(None, T9_REDUCE_COMBINE=1),
    "lds1024": cfg(1024, T9_LDS_SLOTS=1024),
    "lds1024-wavecomb": cfg(1024, T9_LDS_SLOTS=1024, T9_REDUCE_WAVECOMB=1),
    "lds2048": cfg(2048, T9_LDS_SLOTS=2048),
    "lds2048-wavecomb": cfg(2048, T9_LDS_SLOTS=2048, T9_REDUCE_WAVECOMB=1),
    "lds4096": cfg(4096, T9_LDS_SLOTS=4096),
    "lds4096-wavecomb": cfg(4096, T9_LDS_SLOTS=4096, T9_REDUCE_WAVECOMB=1),
    "lds8192": cfg(8192, T9_LDS_SLOTS=8192),
    "lds8192-wavecomb": cfg(8192, T9_LDS_SLOTS=8192, T9_REDUCE_WAVECOMB=1),
    "lds4096-rf0": cfg(4096, T9_LDS_SLOTS=4096, T9_REDUCE_READFIRST=0),
    "lds4096-rf0-wavecomb": cfg(4096, T9_LDS_SLOTS=4096,
                                T9_REDUCE_READFIRST=0, T9_REDUCE_WAVECOMB=1),
}
K128_CFGS = {
    "lds4096-rf": cfg(4096, T9_LDS128_SLOTS=4096),
    "lds4096-rf0": cfg(4096, T9_LDS128_SLOTS=4096, T9_R128_READFIRST=0),
    "lds2048-rf": cfg(2048, T9_LDS128_SLOTS=2048),
    "lds2048-rf0": cfg(2048, T9_LDS128_SLOTS=2048, T9_R128_READFIRST=0),
    "lds1024": cfg(1024, T9_LDS128_SLOTS=1024),
    "stride4-lds4096-rf": cfg(4096, T9_LDS128_SLOTS=4096, T9_R128_STRIDE=4),
}
K128_REFUSED = {
    "stride4-rf0": cfg(4096, T9_R128_STRIDE=4, T9_R128_READFIRST=0),
    "stride4-lds1024": cfg(1024, T9_R128_STRIDE=4, T9_LDS128_SLOTS=1024),
    "stride4-lds2048": cfg(2048, T9_R128_STRIDE=4, T9_LDS128_SLOTS=2048),
}
# the operator path: (SUM, U64), (MIN, I64), (MAX, F64) at 1024 and 4096
# filter slots, read-first on and off
OPS = {"sum-u64": (SUM, U64), "min-i64": (MIN, I64), "max-f64": (MAX, F64)}
OP_CFGS = {
    f"{o}-lds{s}-rf{r}": dict(
        cfg(s, T9_LDS_SLOTS=s, T9_LDS128_SLOTS=s, T9_REDUCE_READFIRST=r,
            T9_R128_READFIRST=r), op=OPS[o])
    for o in OPS for s in (1024, 4096) for r in (1, 0)}
DEFAULT_IDS = ["lds4096", "lds4096-rf", "stride4-lds4096-rf"]


def by_id(cfgs):
    return pytest.mark.parametrize("c", [pytest.param(v, id=k)
                                         for k, v in cfgs.items()])


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


@pytest.fixture()
def knobs(monkeypatch):
    """select(c, grid=None): exactly the knobs of config c and the grid."""
    def select(c, grid=None):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in c["env"].items():
            monkeypatch.setenv(k, v)
        if grid is not None:
            monkeypatch.setenv("T9_REDUCE_GRID", str(grid))
    return select


def next_pow2(n):
    return 1 << max(0, int(n) - 1).bit_length()


def wsum(v):
    return np.add.reduce(R.u64(v)) if len(v) else np.uint64(0)


def slots_of(c):
    return c["slots"] or R.RED_LDS_DEFAULT


def stride_of(c):
    return 4 if c["env"].get("T9_R128_STRIDE") == "4" else 3


# ------------------------------------------------------------- the harness

def scalars():
    return U.garbage(1 + U.NCAN, np.uint32), U.garbage(1 + U.NCAN, np.uint64)


def read_scalar(t, dtype):
    h = U.G.host(t, dtype)
    assert np.all(h[1:] == U.CANARY[dtype]), "wrote behind the scalar"
    return int(h[0])


def run_u64(nat, stream, builds, cap, salt, op=None, refill=None):
    """init, one build per (keys, vals) of `builds` with no init between
    them, raw table, drain. `refill(raw)` may add one more build that
    depends on the table so far. Returns (raw, drained keys, drained
    vals, [d_error after each build])."""
    tail = () if op is None else op
    sfx = "" if op is None else "_op"
    tbl = U.Out(2 * (cap + 1), np.uint64)
    derr, dn = scalars()
    getattr(nat, "reduce_init" + sfx)(tbl.ptr, cap, *tail, stream)
    errs = []
    builds = list(builds)
    while builds:
        keys, vals = builds.pop(0)
        dk, dv = U.In(keys), U.In(vals)
        derr[:1].fill_(-1)                 # every build starts from garbage
        getattr(nat, "reduce_build" + sfx)(dk.ptr, dv.ptr, len(keys),
                                           tbl.ptr, cap, salt, *tail,
                                           derr.data_ptr(), stream)
        U.sync()
        errs.append(read_scalar(derr, np.uint32))
        dk.check()
        dv.check()
        if not builds and refill is not None:
            builds.append(refill(tbl.read().copy()))
            refill = None
    raw = tbl.read().copy()
    ok, ov = U.Out(cap + 1, np.uint64), U.Out(cap + 1, np.uint64)
    getattr(nat, "reduce_drain" + sfx)(tbl.ptr, cap, *tail, ok.ptr, ov.ptr,
                                       dn.data_ptr(), stream)
    U.sync()
    m = read_scalar(dn, np.uint64)
    assert m <= cap + 1
    gk, gv = ok.read(valid=m), ov.read(valid=m)
    assert np.array_equal(tbl.read(), raw), "drain changed the table"
    return raw, gk, gv, errs


def verify_u64(res, cap, salt, keys, vals, op=None):
    """drained multiset, raw table and aux slot against the references."""
    raw, gk, gv, errs = res
    assert errs == [0] * len(errs), errs
    keys, vals = R.u64(keys), R.u64(vals)
    if op is None:
        ek, ev = R.reduce_sum(keys, vals)
    else:
        ek, ev = expected(keys, vals, *op)
    order = np.argsort(gk, kind="stable")
    assert np.array_equal(gk[order], ek)
    assert np.array_equal(gv[order], ev)
    body = ek != M64
    tk, tv = R.check_table_u64(raw, cap, salt)
    assert np.array_equal(tk, ek[body])
    sent = keys == M64
    assert int(raw[2 * cap]) == int(sent.sum()), "aux occurrence count"
    if op is None:
        assert np.array_equal(tv, ev[body])
        assert raw[2 * cap + 1] == wsum(vals[sent]), "aux sum"
    elif op == (SUM, U64):
        assert np.array_equal(tv, ev[body])


def run_128(nat, stream, builds, cap, salt, stride=3, op=None):
    """the same for the 128-bit table; builds are (k1, k2, vals or None).
    Also returns the table buffer, for lookups."""
    tail = () if op is None else op
    sfx = "" if op is None else "_op"
    assert nat.reduce128_table_words(cap) == stride * cap
    tbl = U.Out(stride * cap, np.uint64)
    derr, dn = scalars()
    getattr(nat, "reduce128_init" + sfx)(tbl.ptr, cap, *tail, stream)
    errs = []
    for k1, k2, vals in builds:
        d1, d2 = U.In(k1), U.In(k2)
        dv = None if vals is None else U.In(vals)
        derr[:1].fill_(-1)
        getattr(nat, "reduce128_build" + sfx)(
            d1.ptr, d2.ptr, None if dv is None else dv.ptr, len(k1),
            tbl.ptr, cap, salt, *tail, derr.data_ptr(), stream)
        U.sync()
        errs.append(read_scalar(derr, np.uint32))
        for d in (d1, d2, dv):
            if d is not None:
                d.check()
    raw = tbl.read().copy()
    o1, o2, ov = (U.Out(cap, np.uint64) for _ in range(3))
    getattr(nat, "reduce128_drain" + sfx)(tbl.ptr, cap, *tail, o1.ptr,
                                          o2.ptr, ov.ptr, dn.data_ptr(),
                                          stream)
    U.sync()
    m = read_scalar(dn, np.uint64)
    assert m <= cap
    g = tuple(o.read(valid=m) for o in (o1, o2, ov))
    assert np.array_equal(tbl.read(), raw), "drain changed the table"
    if stride == 4:
        # the payload started as canary: the unused 4th word of every slot
        # must have survived init, build and drain
        assert np.all(raw.reshape(cap, 4)[:, 3] == U.CANARY[np.uint64])
    return raw, g, errs, tbl


def expected_128(k1, k2, vals, op):
    if op is None:
        return R.reduce128_sum(k1, k2, vals)
    pairs, inv = np.unique(np.stack([R.u64(k1), R.u64(k2)], axis=1),
                           axis=0, return_inverse=True)
    vals = np.ones(len(k1), np.uint64) if vals is None else vals
    idx, ev = expected(inv.reshape(-1).astype(np.uint64), vals, *op)
    assert np.array_equal(idx, np.arange(len(pairs)))
    return pairs[:, 0], pairs[:, 1], ev


def verify_128(res, cap, salt, k1, k2, vals, stride=3, op=None):
    raw, (g1, g2, gv), errs, _ = res
    assert errs == [0] * len(errs), errs
    e1, e2, ev = expected_128(k1, k2, vals, op)
    order = np.lexsort((g2, g1))
    assert np.array_equal(g1[order], e1)
    assert np.array_equal(g2[order], e2)
    assert np.array_equal(gv[order], ev)
    t1, t2, tv = R.check_table_128(raw, cap, salt, stride)
    assert np.array_equal(t1, e1) and np.array_equal(t2, e2)
    if op is None or op == (SUM, U64):
        assert np.array_equal(tv, ev)


def check_lookup(nat, stream, res, cap, salt, stride, q1, q2):
    """every query answers the slot where the raw table holds the pair,
    or 0xFFFFFFFF."""
    raw, _, _, tbl = res
    t = raw.reshape(cap, stride)
    where = {(int(a), int(b)): s for s, (a, b) in enumerate(t[:, :2])
             if a != M64}
    exp = np.array([where.get((int(a), int(b)), 0xFFFFFFFF)
                    for a, b in zip(q1, q2)], np.uint32)
    d1, d2 = U.In(q1), U.In(q2)
    out = U.Out(len(q1), np.uint32)
    nat.reduce128_lookup(d1.ptr, d2.ptr, len(q1), tbl.ptr, cap, salt,
                         out.ptr, stream)
    U.sync()
    assert np.array_equal(out.read(), exp)
    assert np.array_equal(tbl.read(), raw), "lookup changed the table"
    d1.check()
    d2.check()
    return exp


# ---------------------------------------------------------------- patterns

def distinct_keys(n, start=1):
    with np.errstate(over="ignore"):
        return np.arange(start, start + n, dtype=np.uint64) * GOLD


def wrapping_vals(rng, n):
    """2^63 + small: a sum of two or more wraps."""
    return np.uint64(1 << 63) + rng.integers(0, 1 << 20, n).astype(np.uint64)


def sentinel_mix(rng, n):
    """keys from {2^64-1, 0, 2^64-2, 2^63}; the sentinel in lane 0 and
    lane 63 of the first wave and in the last lane of the last (partial)
    wave; values include 0."""
    keys = rng.choice(np.array([ONES, 0, ONES - 1, 1 << 63], np.uint64), n)
    vals = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    vals[rng.random(n) < 0.25] = 0
    for at in (0, 63, n - 1):
        if 0 <= at < n:
            keys[at] = M64
    return keys, vals


def chain_u64(rng, salt, slots):
    """the chain keys, each repeated 3-40 times and shuffled, sentinel
    pairs interleaved; cap 16."""
    c = R.colliding_keys(salt, slots, slots - 2, 16, 14, 12)
    keys = np.concatenate([np.repeat(c, rng.integers(3, 41, len(c))),
                           np.full(17, M64)])
    rng.shuffle(keys)
    return c, keys, rng.integers(0, 1 << 64, len(keys), dtype=np.uint64)


def chain_128(rng, salt, slots):
    c = R.colliding_keys(salt, slots, slots - 2, 16, 14, 6)
    k1 = np.concatenate([np.full(8, c[0]), c[1:5]])
    k2 = np.concatenate([np.arange(8, dtype=np.uint64),
                         np.zeros(4, np.uint64)])
    rep = np.repeat(np.arange(12), rng.integers(3, 41, 12))
    rng.shuffle(rep)
    # absent: a present k1 with another k2, and a colliding k1 never built
    absent = (np.array([c[0], c[5]], np.uint64), np.array([99, 0], np.uint64))
    return (k1, k2), k1[rep], k2[rep], absent


def skewed_ids(rng, n, distinct):
    """every id once, the rest drawn with a geometric head."""
    ids = np.concatenate([np.arange(distinct),
                          np.minimum(rng.geometric(0.02, n - distinct) - 1,
                                     distinct - 1)])
    rng.shuffle(ids)
    return ids


def k2_of(k1):
    with np.errstate(over="ignore"):
        return (R.u64(k1) * np.uint64(0xC2B2AE3D27D4EB4F)) >> np.uint64(1)


# ---------------------------------------------------------- u64 table tests

def one_u64(nat, stream, cap, salt, keys, vals, op=None):
    res = run_u64(nat, stream, [(keys, vals)], cap, salt, op)
    verify_u64(res, cap, salt, keys, vals, op)
    return res


def big_sizes(cid):
    """a second trip of the full grid: for the default LDS variants and
    for the two k_reduce_build schedules."""
    if cid in DEFAULT_IDS:
        return [R.RED_BUILD_GRID_CAP * 256 + 1]
    if cid.startswith("combine"):
        return [R.GRID_FOR_CAP * 256 + 1]
    return []


@by_id(U64_CFGS)
def test_u64_shapes(nat, stream, knobs, c, request):
    rng = np.random.default_rng(1)
    few = np.concatenate([distinct_keys(7), [M64]])
    for grid in GRIDS:
        knobs(c, grid)
        for salt in SALTS:
            for n in NS:
                at = (grid, salt, n)
                # one key takes everything; the sum wraps many times
                one_u64(nat, stream, 16, salt,
                        np.full(n, 0x1234567 + n, np.uint64),
                        wrapping_vals(rng, n))
                # all distinct
                one_u64(nat, stream, 2 * next_pow2(n), salt,
                        distinct_keys(n),
                        rng.integers(0, 1 << 64, n, dtype=np.uint64))
                # sentinel mix
                keys, vals = sentinel_mix(rng, n)
                one_u64(nat, stream, 16, salt, keys, vals)
                # all values 0: occupancy is decided by the key word
                keys = few[rng.integers(0, len(few), n)]
                _, gk, gv, _ = one_u64(nat, stream, 16, salt, keys,
                                       np.zeros(n, np.uint64))
                assert len(gk) == len(np.unique(keys)), at
                assert not np.any(gv), at
    knobs(c)
    for n in big_sizes(request.node.callspec.id):
        pool = np.concatenate([distinct_keys(3000),
                               np.array([ONES, 0, ONES - 1], np.uint64)])
        keys = pool[rng.integers(0, len(pool), n)]
        keys[[0, 63, n - 1]] = M64
        vals = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        for salt in SALTS:
            one_u64(nat, stream, 8192, salt, keys, vals)


@by_id(U64_CFGS)
def test_u64_sentinel_only(nat, stream, knobs, c):
    rng = np.random.default_rng(2)
    for grid in GRIDS:
        knobs(c, grid)
        for n in (1, 64, 257):
            keys = np.full(n, M64)
            raw, gk, gv, _ = one_u64(nat, stream, 16, 1, keys,
                                     wrapping_vals(rng, n))
            assert len(gk) == 1 and gk[0] == M64
            assert np.all(raw[0:32:2] == M64) and not np.any(raw[1:32:2])


CHAIN_SLOTS = [14, 15] + list(range(10))   # 12 keys from home slot 14 of 16


@by_id(U64_CFGS)
def test_u64_lds_chain_with_wrap(nat, stream, knobs, c):
    rng = np.random.default_rng(3)
    for grid in (1, 3):
        knobs(c, grid)
        for salt in SALTS:
            ck, keys, vals = chain_u64(rng, salt, slots_of(c))
            raw, _, _, _ = one_u64(nat, stream, 16, salt, keys, vals)
            occ = np.flatnonzero(raw[0:32:2] != M64)
            assert sorted(occ.tolist()) == sorted(CHAIN_SLOTS)


@by_id(U64_CFGS)
def test_u64_exactly_full(nat, stream, knobs, c):
    rng = np.random.default_rng(4)
    knobs(c)
    for cap in (1, 2, 16, 1024):
        for salt in SALTS:
            keys = np.repeat(distinct_keys(cap), 2)
            rng.shuffle(keys)
            vals = rng.integers(0, 1 << 64, len(keys), dtype=np.uint64)
            raw, gk, _, _ = one_u64(nat, stream, cap, salt, keys, vals)
            assert len(gk) == cap and np.all(raw[0:2 * cap:2] != M64)
            # with the sentinel: cap + 1 entries fill the output exactly
            keys = np.concatenate([keys, [M64, M64]])
            rng.shuffle(keys)
            vals = np.concatenate([vals, vals[:2]])
            _, gk, _, _ = one_u64(nat, stream, cap, salt, keys, vals)
            assert len(gk) == cap + 1


@by_id(U64_CFGS)
def test_u64_overflow_by_one_key(nat, stream, knobs, c):
    knobs(c)
    for cap in (1, 2, 16, 1024):
        keys = distinct_keys(cap + 1)

        def again(raw):
            # the keys that made it are re-inserted: no overflow this time
            got = raw[0:2 * cap:2]
            assert np.all(got != M64) and np.all(np.isin(got, keys))
            return got.copy(), np.ones(cap, np.uint64)

        # the call returns and the harness finds every canary intact
        _, gk, _, errs = run_u64(nat, stream, [(keys, keys)], cap, 1,
                                 refill=again)
        # d_error tells of its own call only
        assert errs == [1, 0], (cap, errs)
        assert len(gk) == cap


@by_id(U64_CFGS)
def test_u64_filter_overflow(nat, stream, knobs, c):
    # one block sees 5000 distinct keys: the hot ones reach the global
    # table through the LDS flush, the cold ones directly
    rng = np.random.default_rng(6)
    knobs(c, 1)
    n, distinct = 20_000, 5000
    keys = distinct_keys(distinct)[skewed_ids(rng, n, distinct)]
    keys[rng.integers(0, n, 20)] = M64
    vals = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    for salt in SALTS:
        one_u64(nat, stream, 1 << 14, salt, keys, vals)


def two_builds_u64(rng):
    ka = np.concatenate([distinct_keys(40), [M64]])[rng.integers(0, 41, 300)]
    kb = np.concatenate([distinct_keys(40, 21),
                         [M64]])[rng.integers(0, 41, 500)]
    ka[0] = kb[-1] = M64
    return ka, kb


@by_id(U64_CFGS)
def test_u64_two_builds_without_an_init(nat, stream, knobs, c):
    rng = np.random.default_rng(7)
    ka, kb = two_builds_u64(rng)
    va = rng.integers(0, 1 << 64, len(ka), dtype=np.uint64)
    vb = rng.integers(0, 1 << 64, len(kb), dtype=np.uint64)
    for grid in (None, 1):
        knobs(c, grid)
        res = run_u64(nat, stream, [(ka, va), (kb, vb)], 128, ONES)
        verify_u64(res, 128, ONES, np.concatenate([ka, kb]),
                   np.concatenate([va, vb]))


# ------------------------------------------------------ 128-bit table tests

def one_128(nat, stream, c, cap, salt, k1, k2, vals, op=None):
    res = run_128(nat, stream, [(k1, k2, vals)], cap, salt, stride_of(c), op)
    verify_128(res, cap, salt, k1, k2, vals, stride_of(c), op)
    return res


@by_id(K128_CFGS)
def test_128_shapes(nat, stream, knobs, c, request):
    rng = np.random.default_rng(11)
    # few k1, each under several k2; 0 and 2^64-2 are ordinary key words
    f1 = np.array([0, ONES - 1, 1 << 63, 5], np.uint64)
    for grid in GRIDS:
        knobs(c, grid)
        for salt in SALTS:
            for n in NS:
                one = np.full(n, 0x1234567 + n, np.uint64)
                one_128(nat, stream, c, 16, salt, one, one,
                        wrapping_vals(rng, n))
                one_128(nat, stream, c, 16, salt, one, one, None)
                d1 = distinct_keys(n)
                one_128(nat, stream, c, 2 * next_pow2(n), salt, d1,
                        k2_of(d1),
                        rng.integers(0, 1 << 64, n, dtype=np.uint64))
                k1 = f1[rng.integers(0, 4, n)]
                k2 = f1[rng.integers(0, 3, n)]
                vals = rng.integers(0, 1 << 64, n, dtype=np.uint64)
                vals[rng.random(n) < 0.25] = 0
                one_128(nat, stream, c, 16, salt, k1, k2, vals)
                one_128(nat, stream, c, 16, salt, k1, k2, None)
                # all values 0: still drained
                _, (g1, _, gv), _, _ = one_128(nat, stream, c, 16, salt, k1,
                                               k2, np.zeros(n, np.uint64))
                assert len(g1) == len(np.unique(np.stack([k1, k2]), axis=1).T)
                assert not np.any(gv)
    knobs(c)
    for n in big_sizes(request.node.callspec.id):
        p1 = distinct_keys(3000)
        ids = rng.integers(0, 3000, n)
        k1, k2 = p1[ids // 8], k2_of(p1)[ids]
        vals = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        for salt in SALTS:
            one_128(nat, stream, c, 8192, salt, k1, k2, vals)
        one_128(nat, stream, c, 8192, 0, k1, k2, None)


@by_id(K128_CFGS)
def test_128_lds_chain_with_wrap_and_lookup(nat, stream, knobs, c):
    rng = np.random.default_rng(13)
    st = stride_of(c)
    for grid in (1, 3):
        knobs(c, grid)
        for salt in SALTS:
            (c1, c2), k1, k2, absent = chain_128(rng, salt, slots_of(c))
            for vals in (rng.integers(0, 1 << 64, len(k1), dtype=np.uint64),
                         None):
                res = one_128(nat, stream, c, 16, salt, k1, k2, vals)
                occ = np.flatnonzero(res[0].reshape(16, st)[:, 0] != M64)
                assert sorted(occ.tolist()) == sorted(CHAIN_SLOTS)
                # present keys, then absent ones whose probe walks the
                # whole chain across the wrap
                got = check_lookup(nat, stream, res, 16, salt, st,
                                   np.concatenate([c1, absent[0]]),
                                   np.concatenate([c2, absent[1]]))
                assert sorted(got[:12].tolist()) == sorted(CHAIN_SLOTS)
                assert np.all(got[12:] == 0xFFFFFFFF)


@by_id(K128_CFGS)
def test_128_exactly_full_and_lookup(nat, stream, knobs, c):
    rng = np.random.default_rng(14)
    knobs(c)
    st = stride_of(c)
    for cap in (1, 2, 16, 1024):
        for salt in SALTS:
            # 8 composites per k1 (fewer when cap is)
            d = distinct_keys(cap)
            u1, u2 = d[np.arange(cap) // 8], k2_of(d)
            rep = np.repeat(np.arange(cap), 2)
            rng.shuffle(rep)
            vals = rng.integers(0, 1 << 64, len(rep), dtype=np.uint64)
            res = one_128(nat, stream, c, cap, salt, u1[rep], u2[rep], vals)
            assert len(res[1][0]) == cap
            # on the full table an absent key ends after cap probes
            got = check_lookup(
                nat, stream, res, cap, salt, st,
                np.concatenate([u1, np.array([u1[0], 12345], np.uint64)]),
                np.concatenate([u2, np.array([77, 0], np.uint64)]))
            assert sorted(got[:cap].tolist()) == list(range(cap))
            assert np.all(got[cap:] == 0xFFFFFFFF)


@by_id(K128_CFGS)
def test_128_overflow_by_one_key(nat, stream, knobs, c):
    knobs(c)
    for cap in (1, 2, 16, 1024):
        d = distinct_keys(cap + 1)
        _, (g1, _, _), errs, _ = run_128(nat, stream, [(d, k2_of(d), None)],
                                         cap, 1, stride_of(c))
        assert errs == [1], (cap, errs)
        assert len(g1) == cap


@by_id(K128_CFGS)
def test_128_filter_overflow(nat, stream, knobs, c):
    rng = np.random.default_rng(16)
    knobs(c, 1)
    n, distinct = 20_000, 5000
    ids = skewed_ids(rng, n, distinct)
    d = distinct_keys(distinct)
    k1, k2 = d[ids // 8], k2_of(d)[ids]
    vals = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    for salt in SALTS:
        one_128(nat, stream, c, 1 << 14, salt, k1, k2, vals)
    one_128(nat, stream, c, 1 << 14, 0, k1, k2, None)


def two_builds_128(rng):
    d = distinct_keys(60)
    ia, ib = rng.integers(0, 40, 300), rng.integers(20, 60, 500)
    return (d[ia // 8], k2_of(d)[ia]), (d[ib // 8], k2_of(d)[ib])


@by_id(K128_CFGS)
def test_128_two_builds_without_an_init(nat, stream, knobs, c):
    rng = np.random.default_rng(17)
    (a1, a2), (b1, b2) = two_builds_128(rng)
    va = rng.integers(0, 1 << 64, len(a1), dtype=np.uint64)
    vb = rng.integers(0, 1 << 64, len(b1), dtype=np.uint64)
    st = stride_of(c)
    for grid in (None, 1):
        knobs(c, grid)
        res = run_128(nat, stream, [(a1, a2, va), (b1, b2, vb)], 128, ONES,
                      st)
        verify_128(res, 128, ONES, np.concatenate([a1, b1]),
                   np.concatenate([a2, b2]), np.concatenate([va, vb]), st)
        res = run_128(nat, stream, [(a1, a2, None), (b1, b2, vb)], 128, 0,
                      st)
        verify_128(res, 128, 0, np.concatenate([a1, b1]),
                   np.concatenate([a2, b2]),
                   np.concatenate([np.ones(len(a1), np.uint64), vb]), st)


@by_id(K128_REFUSED)
def test_128_stride4_without_a_stride4_build_is_refused(nat, stream, knobs,
                                                        c):
    # the table is sized for the 4-word stride all the same
    knobs(c)
    d = distinct_keys(300)
    with pytest.raises(T9Error, match="rc=-22"):
        run_128(nat, stream, [(d, k2_of(d), None)], 1024, 0, 4)


# ------------------------------------------- the operator path, same edges

@by_id(OP_CFGS)
def test_op_u64_edges(nat, stream, knobs, c):
    op = c["op"]
    rng = np.random.default_rng(21)
    # LDS chain with wrap
    for grid in (1, 3):
        knobs(c, grid)
        for salt in SALTS:
            _, keys, _ = chain_u64(rng, salt, c["slots"])
            vals = random_bits(rng, len(keys), op[1])
            raw, _, _, _ = one_u64(nat, stream, 16, salt, keys, vals, op)
            occ = np.flatnonzero(raw[0:32:2] != M64)
            assert sorted(occ.tolist()) == sorted(CHAIN_SLOTS)
    knobs(c)
    # exactly full, with the sentinel, and one key too many
    for cap in (1, 2, 16, 1024):
        keys = np.concatenate([np.repeat(distinct_keys(cap), 2), [M64, M64]])
        rng.shuffle(keys)
        vals = random_bits(rng, len(keys), op[1])
        _, gk, _, _ = one_u64(nat, stream, cap, 1, keys, vals, op)
        assert len(gk) == cap + 1
        keys = distinct_keys(cap + 1)
        _, gk, _, errs = run_u64(nat, stream, [(keys, keys)], cap, 1, op)
        assert errs == [1] and len(gk) == cap
    # two builds
    ka, kb = two_builds_u64(rng)
    va, vb = (random_bits(rng, len(k), op[1]) for k in (ka, kb))
    res = run_u64(nat, stream, [(ka, va), (kb, vb)], 128, ONES, op)
    verify_u64(res, 128, ONES, np.concatenate([ka, kb]),
               np.concatenate([va, vb]), op)


@by_id(OP_CFGS)
def test_op_128_edges(nat, stream, knobs, c):
    op = c["op"]
    rng = np.random.default_rng(22)
    for grid in (1, 3):
        knobs(c, grid)
        for salt in SALTS:
            (c1, c2), k1, k2, absent = chain_128(rng, salt, c["slots"])
            vals = random_bits(rng, len(k1), op[1])
            res = one_128(nat, stream, c, 16, salt, k1, k2, vals, op)
            got = check_lookup(nat, stream, res, 16, salt, 3,
                               np.concatenate([c1, absent[0]]),
                               np.concatenate([c2, absent[1]]))
            assert sorted(got[:12].tolist()) == sorted(CHAIN_SLOTS)
            assert np.all(got[12:] == 0xFFFFFFFF)
    knobs(c)
    for cap in (1, 2, 16, 1024):
        d = distinct_keys(cap)
        rep = np.repeat(np.arange(cap), 2)
        rng.shuffle(rep)
        vals = random_bits(rng, len(rep), op[1])
        res = one_128(nat, stream, c, cap, 1, d[rep // 8], k2_of(d)[rep],
                      vals, op)
        assert len(res[1][0]) == cap
        d = distinct_keys(cap + 1)
        _, (g1, _, _), errs, _ = run_128(
            nat, stream, [(d, k2_of(d), d)], cap, 1, 3, op)
        assert errs == [1] and len(g1) == cap
    (a1, a2), (b1, b2) = two_builds_128(rng)
    va, vb = (random_bits(rng, len(k), op[1]) for k in (a1, b1))
    res = run_128(nat, stream, [(a1, a2, va), (b1, b2, vb)], 128, ONES, 3,
                  op)
    verify_128(res, 128, ONES, np.concatenate([a1, b1]),
               np.concatenate([a2, b2]), np.concatenate([va, vb]), 3, op)


# ------------------------------------------------ callers size by the query

def wordcount_triples(n, vocab):
    from thrill_amd.pipeline import WordCount
    wc = WordCount(n, vocab, 1.1, seed=5, rank=0, world=1, device=0)
    try:
        assert wc.keys128
        wc.generate()
        k1, k2, v, m = wc.step()
        g = [U.G.host(t, np.uint64)[:m] for t in (k1, k2, v)]
        words = wc.d_tbl.numel()
    finally:
        wc.close()
    order = np.lexsort((g[1], g[0]))
    return [a[order] for a in g], words


def test_wordcount_sizes_its_table_by_the_stride_knob(nat, oracle, knobs):
    from thrill_amd.pipeline import zipf_cdf
    n, vocab = 1 << 16, 5000
    toks = oracle.zipf_tokens(zipf_cdf(vocab, 1.1), n, seed=5)
    exp = R.reduce128_sum(*R.hash2_of(toks))
    knobs({"env": {}})
    plain, words3 = wordcount_triples(n, vocab)
    knobs({"env": {"T9_R128_STRIDE": "4"}})
    padded, words4 = wordcount_triples(n, vocab)
    assert 3 * words4 == 4 * words3
    for e, a, b in zip(exp, plain, padded):
        assert np.array_equal(a, e) and np.array_equal(b, e)
