"""GPU parity tests of the reduce operators (t9_reduce_*_op,
t9_reduce128_*_op, t9_reduce_by_index_op, pipeline.ReducePairs): SUM, MIN
and MAX over u64, i64 and f64 values.

The oracle only sums, so the expected MIN/MAX results come from NumPy:
sort by key, then np.minimum/np.maximum.reduceat on the typed view. F64
uses the IEEE-754 totalOrder of the bit patterns (-NaN < -inf < ... < -0.0
< +0.0 < ... < +inf < +NaN), restated on the host in enc_f64/dec_f64.
Parity is bit-exact: the three orders are total, so no interleaving of the
atomics can change a result.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tests import _gpu as G
    from thrill_amd import Native, T9Error

SUM, MIN, MAX = 0, 1, 2
U64, I64, F64 = 0, 1, 2
ALLOWED = [(SUM, U64), (SUM, I64), (MIN, U64), (MIN, I64), (MIN, F64),
           (MAX, U64), (MAX, I64), (MAX, F64)]
ONES = np.uint64(2**64 - 1)
MSB = np.uint64(1 << 63)


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = Native(device=0)
    yield n
    n.close()


def enc_f64(bits):
    """totalOrder of f64 bit patterns as unsigned order."""
    neg = (bits >> np.uint64(63)).astype(bool)
    return np.where(neg, ~bits, bits ^ MSB)


def dec_f64(e):
    pos = (e >> np.uint64(63)).astype(bool)
    return np.where(pos, e ^ MSB, ~e)


def fold_groups(vals, starts, op, vtype):
    """fold the key-sorted u64 bit patterns `vals` per group."""
    if op == SUM:
        return np.add.reduceat(vals, starts)        # wrapping u64 add
    f = np.minimum if op == MIN else np.maximum
    if vtype == U64:
        return f.reduceat(vals, starts)
    if vtype == I64:
        return f.reduceat(vals.view(np.int64), starts).view(np.uint64)
    return dec_f64(f.reduceat(enc_f64(vals), starts))


def expected(keys, vals, op, vtype):
    """(sorted unique keys, folded value bit patterns) by NumPy."""
    if len(keys) == 0:
        return np.empty(0, np.uint64), np.empty(0, np.uint64)
    order = np.argsort(keys, kind="stable")
    sk, sv = keys[order], vals[order]
    uk, starts = np.unique(sk, return_index=True)
    return uk, fold_groups(sv, starts, op, vtype)


def random_bits(rng, n, vtype):
    """full-width value bit patterns: negatives for I64; finite doubles
    plus +-0.0, +-inf and denormals for F64."""
    bits = rng.integers(0, 2**64, n, dtype=np.uint64)
    if vtype != F64 or n == 0:
        return bits
    expo = (bits >> np.uint64(52)) & np.uint64(0x7FF)
    bits = np.where(expo == 0x7FF, bits ^ (np.uint64(1) << np.uint64(62)),
                    bits)                             # finite only
    special = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324,
                        2.2e-308 / 4, -2.2e-308 / 4],
                       dtype=np.float64).view(np.uint64)
    pos = rng.choice(n, size=min(n, 8 * len(special)), replace=False)
    bits[pos] = np.resize(special, len(pos))
    return bits


def run_op(nat, keys, vals, cap, op, vtype, salt=0, check_err=True):
    """init_op + build_op + drain_op; returns key-sorted (keys, vals)."""
    n = len(keys)
    dk, dv = G.dev(keys), G.dev(vals)
    tbl = G.empty(2 * (cap + 1), np.uint64)
    derr, dn = G.empty(1, np.uint32), G.empty(1, np.uint64)
    ok, ov = G.empty(cap + 1, np.uint64), G.empty(cap + 1, np.uint64)
    s = G.stream()
    nat.reduce_init_op(G.ptr(tbl), cap, op, vtype, s)
    nat.reduce_build_op(G.ptr(dk), G.ptr(dv), n, G.ptr(tbl), cap, salt, op,
                        vtype, G.ptr(derr), s)
    nat.reduce_drain_op(G.ptr(tbl), cap, op, vtype, G.ptr(ok), G.ptr(ov),
                        G.ptr(dn), s)
    if check_err:
        assert int(G.host(derr, np.uint32)[0]) == 0, "table overflow"
    m = int(G.host(dn, np.uint64)[0])
    gk, gv = G.host(ok, np.uint64)[:m], G.host(ov, np.uint64)[:m]
    order = np.argsort(gk)
    return gk[order], gv[order]


def run_legacy(nat, keys, vals, cap):
    """the plain (sum-only) entry points on the same input."""
    dk, dv = G.dev(keys), G.dev(vals)
    tbl = G.empty(2 * (cap + 1), np.uint64)
    derr, dn = G.empty(1, np.uint32), G.empty(1, np.uint64)
    ok, ov = G.empty(cap + 1, np.uint64), G.empty(cap + 1, np.uint64)
    s = G.stream()
    nat.reduce_init(G.ptr(tbl), cap, s)
    nat.reduce_build(G.ptr(dk), G.ptr(dv), len(keys), G.ptr(tbl), cap, 0,
                     G.ptr(derr), s)
    nat.reduce_drain(G.ptr(tbl), cap, G.ptr(ok), G.ptr(ov), G.ptr(dn), s)
    m = int(G.host(dn, np.uint64)[0])
    gk, gv = G.host(ok, np.uint64)[:m], G.host(ov, np.uint64)[:m]
    order = np.argsort(gk)
    return gk[order], gv[order]


def assert_parity(nat, keys, vals, cap, op, vtype):
    gk, gv = run_op(nat, keys, vals, cap, op, vtype)
    ek, ev = expected(keys, vals, op, vtype)
    assert np.array_equal(gk, ek)
    assert np.array_equal(gv, ev)


# ------------------------------ u64 table ------------------------------

@pytest.mark.parametrize("op,vtype", ALLOWED)
def test_parity_u64_table(nat, oracle, op, vtype):
    rng = np.random.default_rng(100 + 3 * op + vtype)
    n = 1 << 16
    keys = rng.integers(0, 3000, n).astype(np.uint64)
    vals = random_bits(rng, n, vtype)
    gk, gv = run_op(nat, keys, vals, 8192, op, vtype)
    ek, ev = expected(keys, vals, op, vtype)
    assert np.array_equal(gk, ek) and np.array_equal(gv, ev)
    if (op, vtype) == (SUM, U64):
        # the _op entry points agree with the oracle and the legacy ones
        ok_, ov_ = oracle.reduce_u64(keys, vals)
        assert np.array_equal(gk, ok_) and np.array_equal(gv, ov_)
        lk, lv = run_legacy(nat, keys, vals, 8192)
        assert np.array_equal(gk, lk) and np.array_equal(gv, lv)


@pytest.mark.parametrize("op,vtype", ALLOWED)
def test_edge_sizes(nat, op, vtype):
    rng = np.random.default_rng(7)
    for n, nkeys in ((0, 1), (1, 1), (64, 1), (257, 40)):
        keys = rng.integers(10, 10 + nkeys, n).astype(np.uint64)
        vals = random_bits(rng, n, vtype)
        assert_parity(nat, keys, vals, 1024, op, vtype)


@pytest.mark.parametrize("op", [MIN, MAX])
@pytest.mark.parametrize("vtype", [U64, I64, F64])
def test_sentinel_and_zero_keys(nat, op, vtype):
    # key 0xFFFF..F is the empty-slot sentinel: reduced in the aux slot
    rng = np.random.default_rng(11)
    n = 600
    keys = rng.choice(np.array([0, 2**64 - 1, 5, 77, 2**64 - 2],
                               dtype=np.uint64), n)
    vals = random_bits(rng, n, vtype)
    gk, gv = run_op(nat, keys, vals, 16, op, vtype)
    ek, ev = expected(keys, vals, op, vtype)
    assert np.array_equal(gk, ek) and np.array_equal(gv, ev)
    assert gk[-1] == ONES and gv[-1] == ev[-1]   # the drained sentinel key


def test_identity_values_do_not_leak(nat):
    # MIN over all-ones and MAX over 0: the results ARE those values
    keys = (np.arange(500, dtype=np.uint64) % np.uint64(7))
    keys[::50] = ONES                                  # aux slot as well
    gk, gv = run_op(nat, keys, np.full(500, ONES), 64, MIN, U64)
    assert np.array_equal(gk, np.unique(keys))
    assert np.all(gv == ONES)
    gk, gv = run_op(nat, keys, np.zeros(500, np.uint64), 64, MAX, U64)
    assert np.array_equal(gk, np.unique(keys))
    assert np.all(gv == 0)


def test_f64_total_order(nat):
    f = lambda *x: np.array(x, dtype=np.float64).view(np.uint64)  # noqa
    pnan = np.uint64(0x7FF8000000000000)
    nnan = np.uint64(0xFFF8000000000000)
    g1 = np.concatenate([[pnan, nnan], f(np.inf, -np.inf, -0.0, 0.0, 1.5)])
    g2 = f(-0.0, 0.0)
    keys = np.array([1] * len(g1) + [2] * len(g2), dtype=np.uint64)
    vals = np.concatenate([g1, g2]).astype(np.uint64)
    gk, gv = run_op(nat, keys, vals, 16, MIN, F64)
    assert gk.tolist() == [1, 2]
    assert gv[0] == nnan and gv[1] == f(-0.0)[0]
    gk, gv = run_op(nat, keys, vals, 16, MAX, F64)
    assert gv[0] == pnan and gv[1] == f(0.0)[0]


@pytest.fixture(scope="module")
def cold_input():
    """the smallest shape where a block sees more distinct keys than its
    LDS table holds (4 blocks x 1024 slots, 20 000 keys): misses go to the
    global table and one key ends up in several blocks' flushes."""
    rng = np.random.default_rng(19)
    n, distinct = 1 << 16, 20_000
    ids = np.concatenate([np.arange(distinct),
                          rng.integers(0, distinct, n - distinct)])
    rng.shuffle(ids)
    keys = ids.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    vals = random_bits(rng, n, I64)
    return keys, vals, {op: expected(keys, vals, op, I64)
                        for op in (MIN, MAX)}


@pytest.mark.parametrize("op", [MIN, MAX])
def test_cold_path_and_flush(nat, cold_input, monkeypatch, op):
    keys, vals, exp = cold_input
    monkeypatch.setenv("T9_REDUCE_GRID", "4")
    monkeypatch.setenv("T9_LDS_SLOTS", "1024")
    gk, gv = run_op(nat, keys, vals, 1 << 16, op, I64)
    assert len(gk) == 20_000
    assert np.array_equal(gk, exp[op][0]) and np.array_equal(gv, exp[op][1])

    # knobs that select variants the op path may lack: the same result, or
    # T9_EINVAL — never a different result
    monkeypatch.setenv("T9_REDUCE_COMBINE", "1")
    monkeypatch.setenv("T9_REDUCE_WAVECOMB", "1")
    monkeypatch.setenv("T9_REDUCE_READFIRST", "0")
    try:
        gk, gv = run_op(nat, keys, vals, 1 << 16, op, I64)
    except T9Error as e:
        assert "rc=-22" in str(e)
    else:
        assert np.array_equal(gk, exp[op][0])
        assert np.array_equal(gv, exp[op][1])


def test_zipf_skew_first_and_last_occurrence(nat, oracle):
    n, vocab = 1 << 18, 10_000
    toks = oracle.zipf_tokens(oracle.zipf_cdf(vocab, 1.1), n, seed=13)
    pos = np.arange(n, dtype=np.uint64)
    uk, first = np.unique(toks, return_index=True)
    _, last_rev = np.unique(toks[::-1], return_index=True)
    gk, gv = run_op(nat, toks, pos, 1 << 15, MIN, U64)
    assert np.array_equal(gk, uk)
    assert np.array_equal(gv, first.astype(np.uint64))
    gk, gv = run_op(nat, toks, pos, 1 << 15, MAX, U64)
    assert np.array_equal(gk, uk)
    assert np.array_equal(gv, (n - 1 - last_rev).astype(np.uint64))


def test_overflow_sets_error_and_terminates(nat):
    n, cap = 10_000, 1024
    keys = np.arange(1, n + 1, dtype=np.uint64)
    dk, dv = G.dev(keys), G.dev(keys)
    tbl = G.empty(2 * (cap + 1), np.uint64)
    derr = G.empty(1, np.uint32)
    s = G.stream()
    nat.reduce_init_op(G.ptr(tbl), cap, MIN, U64, s)
    nat.reduce_build_op(G.ptr(dk), G.ptr(dv), n, G.ptr(tbl), cap, 0, MIN,
                        U64, G.ptr(derr), s)
    assert int(G.host(derr, np.uint32)[0]) == 1


# ----------------------------- 128-bit table ---------------------------

def run_op128(nat, k1, k2, vals, cap, op, vtype, salt=0, slot_u64s=3):
    n = len(k1)
    d1, d2, dv = G.dev(k1), G.dev(k2), G.dev(vals)
    tbl = G.empty(slot_u64s * cap, np.uint64)
    derr, dn = G.empty(1, np.uint32), G.empty(1, np.uint64)
    o1, o2, ov = (G.empty(cap, np.uint64) for _ in range(3))
    s = G.stream()
    nat.reduce128_init_op(G.ptr(tbl), cap, op, vtype, s)
    nat.reduce128_build_op(G.ptr(d1), G.ptr(d2), G.ptr(dv), n, G.ptr(tbl),
                           cap, salt, op, vtype, G.ptr(derr), s)
    nat.reduce128_drain_op(G.ptr(tbl), cap, op, vtype, G.ptr(o1), G.ptr(o2),
                           G.ptr(ov), G.ptr(dn), s)
    assert int(G.host(derr, np.uint32)[0]) == 0, "table overflow"
    m = int(G.host(dn, np.uint64)[0])
    g1, g2, gv = (G.host(t, np.uint64)[:m] for t in (o1, o2, ov))
    order = np.lexsort((g2, g1))
    return g1[order], g2[order], gv[order], (tbl, o1, o2, m)


@pytest.fixture(scope="module")
def input128():
    rng = np.random.default_rng(23)
    n = 1 << 16
    ids = rng.integers(0, 5000, n).astype(np.uint64)
    k1 = ids * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1)
    k2 = (ids * np.uint64(0xC2B2AE3D27D4EB4F)) ^ np.uint64(7)
    vals = random_bits(rng, n, I64)
    exp = {}
    for op in (MIN, MAX):
        # k2 is a function of k1 here, so grouping on k1 is the composite
        uk1, ev = expected(k1, vals, op, I64)
        _, idx = np.unique(k1, return_index=True)
        exp[op] = (uk1, k2[idx], ev)
    return k1, k2, vals, exp


@pytest.mark.parametrize("op", [MIN, MAX])
def test_parity_128(nat, input128, op):
    k1, k2, vals, exp = input128
    g1, g2, gv, _ = run_op128(nat, k1, k2, vals, 1 << 14, op, I64)
    assert np.array_equal(g1, exp[op][0])
    assert np.array_equal(g2, exp[op][1])
    assert np.array_equal(gv, exp[op][2])


def test_forced_k1_collision_keeps_separate_minima(nat):
    rng = np.random.default_rng(29)
    n = 4000
    k1 = np.full(n, 0x1234, dtype=np.uint64)
    k1[::5] = 99
    k2 = np.where(np.arange(n) % 2 == 0, np.uint64(10), np.uint64(20))
    vals = rng.integers(1000, 1 << 50, n).astype(np.uint64)
    g1, g2, gv, _ = run_op128(nat, k1, k2, vals, 64, MIN, U64)
    acc = {}
    for a, b, v in zip(k1.tolist(), k2.tolist(), vals.tolist()):
        acc[(a, b)] = min(acc.get((a, b), v), v)
    assert len(acc) == 4
    assert sorted(acc.items()) == [
        ((a, b), v) for a, b, v in zip(g1.tolist(), g2.tolist(),
                                       gv.tolist())]


def test_lookup_finds_every_key_of_a_min_built_table(nat, input128):
    k1, k2, vals, exp = input128
    cap = 1 << 14
    g1, g2, gv, (tbl, o1, o2, m) = run_op128(nat, k1, k2, vals, cap, MIN,
                                             I64)
    dslot = G.empty(m, np.uint32)
    nat.reduce128_lookup(G.ptr(o1), G.ptr(o2), m, G.ptr(tbl), cap, 0,
                         G.ptr(dslot), G.stream())
    slot = G.host(dslot, np.uint32)
    assert np.all(slot < cap)
    assert len(np.unique(slot)) == m
    t = G.host(tbl, np.uint64).reshape(cap, 3)
    assert np.array_equal(t[slot, 0], G.host(o1, np.uint64)[:m])
    assert np.array_equal(t[slot, 1], G.host(o2, np.uint64)[:m])


def test_stride4_refused_or_correct(nat, input128, monkeypatch):
    k1, k2, vals, exp = input128
    monkeypatch.setenv("T9_R128_STRIDE", "4")
    try:
        g1, g2, gv, _ = run_op128(nat, k1, k2, vals, 1 << 14, MIN, I64,
                                  slot_u64s=4)   # table sized for stride 4
    except T9Error as e:
        assert "rc=-22" in str(e)
    else:
        assert np.array_equal(g1, exp[MIN][0])
        assert np.array_equal(g2, exp[MIN][1])
        assert np.array_equal(gv, exp[MIN][2])


# ------------------------------- by index ------------------------------

# raw bit pattern of each operator's identity per value type
IDENT = {(MIN, U64): 2**64 - 1, (MIN, I64): 2**63 - 1,
         (MAX, U64): 0, (MAX, I64): 1 << 63}


def run_by_index(nat, keys, vals, begin, size, op, vtype, neutral):
    dk, dv = G.dev(keys), G.dev(vals)
    dd, de = G.empty(size, np.uint64), G.empty(1, np.uint32)
    w = G.ws(nat.ws("reduce_by_index_op", size))
    nat.reduce_by_index_op(G.ptr(dk), G.ptr(dv), len(keys), begin, size, op,
                           vtype, neutral, G.ptr(dd), G.ptr(de), G.ptr(w),
                           G.stream())
    return G.host(dd, np.uint64), int(G.host(de, np.uint32)[0])


@pytest.mark.parametrize("op", [MIN, MAX])
@pytest.mark.parametrize("vtype", [U64, I64])
def test_by_index(nat, op, vtype):
    rng = np.random.default_rng(31 + 2 * op + vtype)
    n, begin, size, neutral = 1 << 18, 1000, 5000, 12345
    idx = rng.integers(0, size, n)
    lone = 4242                         # receives only the identity value
    keep = (idx % 10 != 7) & (idx != lone)   # a tenth of the indices empty
    idx = idx[keep]
    vals = random_bits(rng, len(idx), vtype)
    idx = np.append(idx, [lone, lone])
    vals = np.append(vals, np.full(2, IDENT[(op, vtype)], dtype=np.uint64))
    keys = (idx + begin).astype(np.uint64)
    got, err = run_by_index(nat, keys, vals, begin, size, op, vtype, neutral)
    assert err == 0
    uk, ev = expected(keys, vals, op, vtype)
    want = np.full(size, neutral, dtype=np.uint64)
    want[(uk - np.uint64(begin)).astype(np.int64)] = ev
    empty = np.arange(size) % 10 == 7
    assert 400 <= empty.sum() <= 600 and np.all(want[empty] == neutral)
    assert want[lone] == IDENT[(op, vtype)]
    assert np.array_equal(got, want)

    # an out-of-range key sets the error flag
    bad = keys.copy()
    bad[17] = begin + size + 3
    _, err = run_by_index(nat, bad, vals, begin, size, op, vtype, neutral)
    assert err == 1
    bad[17] = begin - 1
    _, err = run_by_index(nat, bad, vals, begin, size, op, vtype, neutral)
    assert err == 1


def test_by_index_sum_matches_legacy_where_touched(nat, oracle):
    rng = np.random.default_rng(37)
    n, begin, size = 1 << 16, 50, 777
    keys = rng.integers(begin, begin + size, n).astype(np.uint64)
    vals = rng.integers(0, 1 << 40, n).astype(np.uint64)
    got, err = run_by_index(nat, keys, vals, begin, size, SUM, U64, 0)
    assert err == 0
    assert np.array_equal(got, oracle.reduce_by_index(keys, vals, begin,
                                                      size))


# ------------------------------- pipeline ------------------------------

@pytest.fixture(scope="module")
def pairs_input():
    rng = np.random.default_rng(41)
    n = 1 << 18
    keys = rng.integers(0, 30_000, n).astype(np.uint64)
    vals = random_bits(rng, n, I64)
    return keys, vals, expected(keys, vals, MIN, I64)


def pipeline_result(keys, vals):
    from thrill_amd.pipeline import ReducePairs
    rp = ReducePairs(MIN, I64, rank=0, world=1, device=0)
    ok, ov, m = rp.step(G.dev(keys), G.dev(vals))
    gk, gv = G.host(ok, np.uint64), G.host(ov, np.uint64)
    rp.close()
    assert m == len(gk)
    order = np.argsort(gk)
    return gk[order], gv[order]


def test_reduce_pairs_pipeline(nat, pairs_input):
    keys, vals, (ek, ev) = pairs_input
    gk, gv = pipeline_result(keys, vals)
    assert np.array_equal(gk, ek) and np.array_equal(gv, ev)


@pytest.fixture()
def dist_world1(monkeypatch):
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29547",
                            rank=0, world_size=1)
    monkeypatch.setenv("T9_FORCE_DIST", "1")
    yield dist
    dist.destroy_process_group()


def test_reduce_pairs_pipeline_distributed_branch(nat, pairs_input,
                                                  dist_world1):
    # pre-reduce -> hash partition -> exchange (loopback) -> post-reduce
    keys, vals, (ek, ev) = pairs_input
    gk, gv = pipeline_result(keys, vals)
    assert np.array_equal(gk, ek) and np.array_equal(gv, ev)
