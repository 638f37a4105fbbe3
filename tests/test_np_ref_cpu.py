"""The numpy references of tests/_np_ref.py are pinned to the CPU oracle on
random and edge inputs, and the kernel geometry they carry is pinned to
the kernel sources: a retuned tile fails here instead of silently moving
the boundary-shape GPU ladders off their edges."""
import os
import re

import numpy as np
import pytest

from tests import _np_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "thrill_amd", "csrc")

ONES = 0xFFFFFFFFFFFFFFFF
EDGE = np.array([0, 1, 2, 255, 256, 1 << 31, (1 << 32) - 1, 1 << 32,
                 (1 << 63) - 1, 1 << 63, (1 << 63) + 1, ONES - 1, ONES],
                dtype=np.uint64)


def rand_u64(rng, n):
    return rng.integers(0, 1 << 64, n, dtype=np.uint64)


# ------------------------------------------------------------------ hashes

def test_hash128to64_matches_oracle(oracle):
    rng = np.random.default_rng(1)
    up = np.concatenate([np.repeat(EDGE, len(EDGE)), rand_u64(rng, 500)])
    lo = np.concatenate([np.tile(EDGE, len(EDGE)), rand_u64(rng, 500)])
    got = R.hash128to64(up, lo)
    exp = np.array([oracle.hash128to64(int(a), int(b))
                    for a, b in zip(up, lo)], dtype=np.uint64)
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("p", [1, 2, 3, 255, 256])
@pytest.mark.parametrize("salt", [0, 1, ONES])
def test_hash_bucket_matches_oracle(oracle, p, salt):
    rng = np.random.default_rng(p)
    keys = np.concatenate([EDGE, rand_u64(rng, 300)])
    exp = np.array([oracle.partition_of_u64(int(k), salt, p) for k in keys],
                   dtype=np.uint32)
    assert np.array_equal(R.hash_bucket(keys, salt, p), exp)


def test_hash2_of_is_two_salted_hashes_without_the_sentinel(oracle):
    rng = np.random.default_rng(2)
    ids = np.concatenate([EDGE, rand_u64(rng, 300)])
    k1, k2 = R.hash2_of(ids)
    for base, k in ((0x9AE16A3B2F90404F, k1), (0xC3A5C85C97CB3127, k2)):
        exp = np.array([oracle.hash128to64(base, int(i)) for i in ids],
                       dtype=np.uint64)
        exp = np.where(exp == np.uint64(ONES), exp ^ np.uint64(1), exp)
        assert np.array_equal(k, exp)
    assert not np.any(k1 == np.uint64(ONES))
    assert not np.any(k2 == np.uint64(ONES))


def test_bucket_mod_is_unsigned():
    keys = np.array([ONES, 1 << 63, (1 << 63) + 5], dtype=np.uint64)
    assert R.bucket_mod(keys, 255).tolist() == [
        ONES % 255, (1 << 63) % 255, ((1 << 63) + 5) % 255]


# ---------------------------------------------------------------- classify

def splitters(rng, keys, p, gidx0, dup=False):
    """p-1 splitters sorted by (key, index): sampled items, or one key
    repeated with ascending indices."""
    m = p - 1
    if m == 0:
        return np.empty(0, np.uint64), np.empty(0, np.uint64)
    if dup:
        sk = np.full(m, keys[len(keys) // 2], np.uint64)
        si = np.sort(rng.integers(0, len(keys) + 2, m).astype(np.uint64))
        si += np.uint64(gidx0)
        return sk, si
    pos = np.sort(rng.integers(0, len(keys), m))
    sk, si = keys[pos], pos.astype(np.uint64) + np.uint64(gidx0)
    order = np.lexsort((si, sk))
    return sk[order], si[order]


@pytest.mark.parametrize("p", [1, 2, 3, 5, 8, 255, 256])
@pytest.mark.parametrize("kind", ["random", "few", "edge", "dupspl"])
def test_classify_matches_oracle_closed_form_and_tree(oracle, p, kind):
    rng = np.random.default_rng(p * 7 + len(kind))
    n, gidx0 = 1500, (1 << 40) + 3
    if kind == "random":
        keys = rand_u64(rng, n)
    elif kind == "few":
        keys = rng.integers(0, 6, n).astype(np.uint64) * np.uint64(1 << 61)
    elif kind == "edge":
        keys = rng.choice(np.array([0, ONES, 1 << 63], np.uint64), n)
    else:
        keys = np.full(n, 77, np.uint64)
    sk, si = splitters(rng, keys, p, gidx0, dup=(kind == "dupspl"))
    got = R.classify(keys, gidx0, sk, si)
    assert np.array_equal(got, oracle.classify_u64(keys, gidx0, sk, si, p))
    assert np.array_equal(
        got, oracle.classify_u64(keys, gidx0, sk, si, p, tree=True))
    assert got.max() <= p - 1


def test_classify_is_strict_on_the_items_own_index(oracle):
    # splitter (k, g) equals item (k, g): not strictly below -> bucket 0;
    # the next item, same key, is above it
    keys = np.array([ONES, ONES, ONES, 0], np.uint64)
    sk, si = np.array([ONES], np.uint64), np.array([101], np.uint64)
    got = R.classify(keys, 100, sk, si)
    assert got.tolist() == [0, 0, 1, 0]
    assert np.array_equal(got, oracle.classify_u64(keys, 100, sk, si, 2))


@pytest.mark.parametrize("rec", [8, 12, 100])
@pytest.mark.parametrize("p", [1, 2, 8, 256])
def test_classify_rec_matches_oracle(oracle, rec, p):
    rng = np.random.default_rng(rec + p)
    n, gidx0 = 700, 1 << 33
    # few distinct records that differ late, bytes on both sides of 0x80
    pool = np.full((6, rec), 0x7F, np.uint8)
    pool[:, rec - 1] = [0x00, 0x7F, 0x80, 0xFF, 0x01, 0xFE]
    pool[4:, 0] = 0x80
    recs = pool[rng.integers(0, len(pool), n)]
    pos = np.sort(rng.integers(0, n, p - 1))
    spl = recs[pos].reshape(p - 1, rec)
    si = pos.astype(np.uint64) + np.uint64(gidx0)
    order = np.lexsort((si,) + tuple(spl[:, j]
                                     for j in range(rec - 1, -1, -1)))
    spl, si = np.ascontiguousarray(spl[order]), si[order]
    got = R.classify_rec(recs, gidx0, spl, si)
    exp = oracle.classify_rec(recs, gidx0, rec, spl if p > 1 else
                              np.zeros((1, rec), np.uint8), si, p)
    assert np.array_equal(got, exp)


# ------------------------------------------------------------ reduce side

@pytest.mark.parametrize("size", [1, 2, 5000])
def test_reduce_by_index_matches_oracle(oracle, size):
    rng = np.random.default_rng(size)
    n, begin = 20_000, 1000
    keys = rng.integers(begin, begin + size, n).astype(np.uint64)
    keys[0], keys[-1] = begin, begin + size - 1
    vals = rand_u64(rng, n)                        # sums wrap
    dense, err = R.reduce_by_index(keys, vals, begin, size)
    assert err == 0
    assert np.array_equal(dense,
                          oracle.reduce_by_index(keys, vals, begin, size))


def test_reduce_by_index_flags_both_sides_and_keeps_the_rest():
    keys = np.array([9, 10, 12, 13, 10, ONES, 0], np.uint64)
    vals = np.array([1, 2, 4, 8, ONES, 16, 32], np.uint64)
    dense, err = R.reduce_by_index(keys, vals, 10, 3)
    assert err == 1
    assert dense.tolist() == [1, 0, 4]             # 2 + (2^64 - 1) wraps
    assert R.reduce_by_index(keys[1:3], vals[1:3], 10, 3)[1] == 0


def test_index_bucket_reference():
    b, err = R.index_bucket(np.array([50, 52, 49, 53, 0], np.uint64),
                            50, 3, 256)
    # cells 0 and 2 of 3 over 256 partitions; outsiders go with cell 2
    assert b.tolist() == [0, 170, 170, 170, 170] and err == 1
    b, err = R.index_bucket(np.arange(7, 1007, dtype=np.uint64), 7, 1000, 3)
    assert err == 0
    assert np.array_equal(b, (np.arange(1000) * 3 // 1000).astype(np.uint32))
    assert R.index_bucket(np.array([0], np.uint64), 0, 1, 256)[0][0] == 0


# ------------------------------------------------ group, partition, merges

def test_group_partition_merge_references_on_small_cases():
    u, o = R.group_index(np.array([0, 0, 3, 3, 3, ONES], np.uint64))
    assert u.tolist() == [0, 3, ONES] and o.tolist() == [0, 2, 5]
    perm, off = R.partition(np.array([2, 0, 2, 0, 3], np.uint32), 5)
    assert perm.tolist() == [1, 3, 0, 2, 4]
    assert off.tolist() == [0, 2, 2, 4, 5, 5]
    assert R.merge([1, 5, ONES], [0, 5]).tolist() == [0, 1, 5, 5, ONES]
    A = np.array([[0, 0, 0, 1], [0, 0, 0, 0x80]], np.uint8)
    B = np.array([[0, 0, 0, 1], [0, 0, 0, 0x7F], [1, 0, 0, 0]], np.uint8)
    assert R.merge_records(A, B)[:, [0, 3]].tolist() == [
        [0, 1], [0, 1], [0, 0x7F], [0, 0x80], [1, 0]]
    rng = np.random.default_rng(3)
    recs = rng.integers(0, 256, (300, 12)).astype(np.uint8)
    exp = sorted(bytes(r) for r in recs)
    assert [bytes(r) for r in R.sort_records(recs)] == exp


# ---------------------------------------------------------------- geometry

def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def define(text, name):
    m = re.search(r"^#define\s+" + name + r"\s+(\d+)\s", text, re.M)
    assert m, f"#define {name} not found"
    return int(m.group(1))


def body_of(text, signature):
    """source text from `signature` to the next line that closes a
    top-level function."""
    at = text.index(signature)
    return text[at:text.index("\n}\n", at)]


def grid_caps(body):
    """every `(x < N) ? ... : N` clamp of a grid in a host function."""
    caps = re.findall(
        r"\(\w+ < (\d+)\) \? (?:\(\w+ \? \w+ : 1\)|\w+) : (\d+)", body)
    assert caps and all(a == b for a, b in caps), caps
    return {int(a) for a, _ in caps}


def test_geometry_constants_match_the_sources():
    grp, mrg = src("t9_group.hip"), src("t9_merge.hip")
    com, srt = src("t9_common.h"), src("t9_sort.hip")
    red, rec = src("t9_reduce.hip"), src("t9_records.hip")
    assert define(grp, "GRP_TILE") == R.GRP_TILE == 8192
    assert define(mrg, "MRG_TILE") == R.MRG_TILE == 4096
    assert define(mrg, "MRG_REC_TILE") == R.MRG_REC_TILE == 1024
    assert define(com, "T9_PAIRS_TILE") == R.PAIRS_TILE == 2048
    assert define(com, "T9_SCAN_CHUNK") == R.SCAN_CHUNK == 32
    # spans per thread: tile / 256 threads
    assert "span = MRG_TILE / 256;" in mrg
    assert "span = MRG_REC_TILE / 256;" in mrg
    assert R.MRG_SPAN == R.MRG_TILE // 256 == 16
    assert R.MRG_REC_SPAN == R.MRG_REC_TILE // 256 == 4
    # k_grp_scan walks the block sums 256 at a time
    assert "for (u64 c = 0; c < B; c += 256)" in grp
    assert R.GRP_SCAN == 256
    # k_chunkscan's unrolled trip
    m = re.search(r"constexpr int U = (\d+);", body_of(srt, "void k_chunkscan("))
    assert m and int(m.group(1)) == R.CHUNKSCAN_UNROLL == 16
    # partition_idx uses the pairs tile
    part = body_of(srt, "int t9_partition_idx(")
    assert "t9_ceil_div(n, T9_PAIRS_TILE)" in part
    # grid caps
    for sig in ("int t9_classify_u64(", "int t9_classify_rec("):
        assert grid_caps(body_of(srt, sig)) == {R.CLASSIFY_GRID_CAP} == {2048}
    assert grid_caps(body_of(red, "u32 grid_for(u64 work)")) == \
        {R.GRID_FOR_CAP} == {4096}
    assert grid_caps(body_of(rec, "u32 grid_for(u64 work)")) == \
        {R.GRID_FOR_CAP}
    for fn in ("t9_hash_bucket", "t9_bucket_mod", "t9_index_bucket",
               "t9_reduce_by_index", "t9_hash2_of"):
        assert "dim3(grid_for(n))" in body_of(red, "int " + fn + "(")
    assert grid_caps(body_of(rec, "int t9_extract_key64_le(")) == \
        {R.RECORDS_GRID_CAP} == {16384}
    m = re.search(r"ecap = eg \? \(u32\)atoi\(eg\) : (\d+);",
                  body_of(rec, "int t9_extract_key64("))
    assert m and int(m.group(1)) == R.RECORDS_GRID_CAP
    m = re.search(r"gcap = gg \? \(u32\)atoi\(gg\) : (\d+);",
                  body_of(rec, "int t9_gather_records("))
    assert m and int(m.group(1)) == R.RECORDS_GRID_CAP


# ------------------------------------------------------ reduce hash tables

def sentinel_bearing(rng, n, distinct):
    """keys from a small set of wide values, the edge keys (sentinel 2^64-1
    included) mixed in."""
    pool = np.concatenate([rand_u64(rng, distinct), EDGE])
    return pool[rng.integers(0, len(pool), n)]


@pytest.mark.parametrize("n,distinct", [(1, 1), (257, 5), (20_000, 3000)])
def test_reduce_sum_matches_oracle(oracle, n, distinct):
    rng = np.random.default_rng(n)
    for keys in (rand_u64(rng, distinct)[rng.integers(0, distinct, n)],
                 sentinel_bearing(rng, n, distinct)):
        vals = rand_u64(rng, n)                    # sums wrap
        gk, gv = R.reduce_sum(keys, vals)
        ek, ev = oracle.reduce_u64(keys, vals)
        assert np.array_equal(gk, ek) and np.array_equal(gv, ev)
    ek, ev = R.reduce_sum([], [])
    assert len(ek) == 0 and len(ev) == 0
    ek, ev = R.reduce_sum([ONES, 5, ONES], [1 << 63, 7, 1 << 63])
    assert ek.tolist() == [5, ONES] and ev.tolist() == [7, 0]


@pytest.mark.parametrize("n,distinct", [(1, 1), (257, 5), (20_000, 3000)])
@pytest.mark.parametrize("with_vals", [True, False])
def test_reduce128_sum_matches_oracle(oracle, n, distinct, with_vals):
    rng = np.random.default_rng(n + 1)
    ids = rng.integers(0, distinct, n)
    # few k1 shared by many k2, so equality has to be on the pair; the
    # reserved all-ones is no legal k1 or k2
    k1 = (rand_u64(rng, 1 + distinct // 8) >> np.uint64(1))[ids // 8]
    k2 = (rand_u64(rng, distinct) >> np.uint64(1))[ids]
    vals = rand_u64(rng, n) if with_vals else None
    got = R.reduce128_sum(k1, k2, vals)
    exp = oracle.reduce128(k1, k2, vals)
    order = np.lexsort((exp[1], exp[0]))
    for g, e in zip(got, exp):
        assert np.array_equal(g, e[order])
    assert all(len(a) == 0 for a in R.reduce128_sum([], [], None))


def test_slot_formulas_and_colliding_keys(oracle):
    rng = np.random.default_rng(5)
    keys = np.concatenate([EDGE, rand_u64(rng, 200)])
    for salt in (0, 1, ONES):
        h = np.array([oracle.hash128to64(salt, int(k)) for k in keys],
                     dtype=np.uint64)
        for cap in (1, 2, 16, 1 << 20):
            assert np.array_equal(R.home_slot(keys, salt, cap),
                                  h & np.uint64(cap - 1))
        for slots in (1024, 2048, 4096, 8192):
            assert np.array_equal(
                R.lds_slot(keys, salt, slots),
                (h >> np.uint64(48)) & np.uint64(slots - 1))
            c = R.colliding_keys(salt, slots, slots - 2, 16, 14, 16)
            assert len(np.unique(c)) == 16 and not np.any(c == R.M64)
            assert np.all(R.lds_slot(c, salt, slots) == slots - 2)
            assert np.all(R.home_slot(c, salt, 16) == 14)


def table_u64(cap, placed, aux=(0, 0)):
    raw = np.zeros(2 * (cap + 1), np.uint64)
    raw[0:2 * cap:2] = R.M64
    for slot, k, v in placed:
        raw[2 * slot], raw[2 * slot + 1] = k, v
    raw[2 * cap], raw[2 * cap + 1] = aux
    return raw


def test_check_table_u64_accepts_chains_and_rejects_broken_ones():
    cap, salt = 16, 1
    c = R.colliding_keys(salt, 4096, 4094, cap, 14, 4)
    # a chain from slot 14 across the wrap to slot 1
    good = table_u64(cap, [(14, c[0], 5), (15, c[1], 6), (0, c[2], 7),
                           (1, c[3], 0)], aux=(3, 9))
    k, v = R.check_table_u64(good, cap, salt)
    order = np.argsort(c)
    assert np.array_equal(k, c[order])
    assert np.array_equal(v, np.array([5, 6, 7, 0], np.uint64)[order])
    # a full table is one unbroken chain
    full = R.colliding_keys(salt, 4096, 4094, cap, 14, 16)
    R.check_table_u64(table_u64(cap, [(i, k, 1) for i, k in
                                      enumerate(full)]), cap, salt)
    with pytest.raises(AssertionError, match="two slots"):
        R.check_table_u64(table_u64(cap, [(14, c[0], 5), (15, c[0], 6)]),
                          cap, salt)
    with pytest.raises(AssertionError, match="empty slot"):
        R.check_table_u64(table_u64(cap, [(14, c[0], 5), (0, c[2], 7)]),
                          cap, salt)
    with pytest.raises(AssertionError, match="empty slot"):
        R.check_table_u64(table_u64(cap, [(13, c[0], 5)]), cap, salt)


@pytest.mark.parametrize("stride", [3, 4])
def test_check_table_128_accepts_chains_and_rejects_broken_ones(stride):
    cap, salt = 16, ONES
    c = R.colliding_keys(salt, 1024, 1022, cap, 14, 2)

    def table(placed):
        t = np.full((cap, stride), 0xAB, np.uint64)
        t[:, 0] = t[:, 1] = R.M64
        t[:, 2] = 0
        for slot, a, b, v in placed:
            t[slot, :3] = a, b, v
        return t.reshape(-1)

    k1, k2, v = R.check_table_128(
        table([(14, c[0], 2, 5), (15, c[0], 1, 6), (0, c[1], 1, 7)]),
        cap, salt, stride)
    exp = sorted([(int(c[0]), 1, 6), (int(c[0]), 2, 5), (int(c[1]), 1, 7)])
    assert list(zip(k1.tolist(), k2.tolist(), v.tolist())) == exp
    with pytest.raises(AssertionError, match="two slots"):
        R.check_table_128(table([(14, c[0], 2, 5), (15, c[0], 2, 6)]),
                          cap, salt, stride)
    with pytest.raises(AssertionError, match="k2 left empty"):
        R.check_table_128(table([(14, c[0], ONES, 0)]), cap, salt, stride)
    with pytest.raises(AssertionError, match="empty slot"):
        R.check_table_128(table([(14, c[0], 2, 5), (0, c[1], 1, 7)]),
                          cap, salt, stride)


def test_reduce_table_geometry_matches_the_sources():
    red, op = src("t9_reduce.hip"), src("t9_reduce_op.hip")
    # the LDS filter's start slot: bits 48.. of the salted hash; one such
    # expression per LDS build kernel
    assert red.count("u32 ls = (u32)(h >> 48) & (T9_LDS_SLOTS - 1);") == 1
    assert red.count("u32 ls = (u32)(h >> 48) & (SLOTS - 1);") == 1
    assert op.count("u32 ls = (u32)(h >> 48) & (SLOTS - 1);") == 2
    # its probe count
    assert red.count("for (int p = 0; p < 4; ++p)") == 2
    assert op.count("for (int p = 0; p < 4; ++p)") == 2
    assert R.RED_LDS_PROBES == 4
    # the home slot: the low bits of the same hash
    assert "u64 slot = h & (cap - 1);" in red
    assert "u64 slot = h & (cap - 1);" in op
    assert "u64 slot = t9_hash128to64(salt, k1) & (cap - 1);" in red
    assert "u64 slot = t9_hash128to64(salt, k1) & (cap - 1);" in op
    # default filter size and the grid clamp of the four build entry points
    for text, fn in ((red, "t9_reduce_build"), (red, "t9_reduce128_build"),
                     (op, "t9_reduce_build_op"),
                     (op, "t9_reduce128_build_op")):
        m = re.search(r"const int slots = se \? atoi\(se\) : (\d+);",
                      body_of(text, "int " + fn + "("))
        assert m and int(m.group(1)) == R.RED_LDS_DEFAULT == 4096, fn
    for fn in ("t9_reduce_build", "t9_reduce128_build"):
        m = re.search(r"if \(!ge && grid > (\d+)\) grid = (\d+);",
                      body_of(red, "int " + fn + "("))
        assert m and int(m.group(1)) == int(m.group(2)) == \
            R.RED_BUILD_GRID_CAP == 1024, fn
    m = re.search(r"\*grid = g > (\d+) \? (\d+) : g;",
                  body_of(op, "bool env_grid("))
    assert m and int(m.group(1)) == int(m.group(2)) == R.RED_BUILD_GRID_CAP
    # the wave pre-combine matches lanes on 11 bits of the LDS slot
    assert "for (int b = 0; b < 11; ++b)" in red
