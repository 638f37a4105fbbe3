"""GPU tests of the device inner join (t9_join_count / t9_join_emit and
pipeline.InnerJoin) against numpy (tests/_join_ref.py). Every comparison is
array_equal on both index arrays. Shapes come from t9_join_geometry: with LT
the left keys per matching block, OT the output positions per emit block and
SK the most right keys a matching block stages in LDS, the cases cross every
tile edge and both search paths. Outputs stay below 2e6 pairs.

Every count runs on a workspace pre-filled with 0xFF bytes, every emit
writes into buffers with guard words behind n_out, and the inputs are
compared with what was uploaded afterwards.

The random 20 000 x 15 000 case draws both sides with
default_rng(1).integers(0, 5000, n, dtype=uint64), left first; that draw has
60 176 matching pairs (the checker's count, asserted below)."""
import os

import numpy as np
import pytest
import torch

from tests import _join_ref as J

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tests import _gpu as G

GUARD = np.uint32(0xC0FFEE42)
NGUARD = 64
TOP = np.uint64(0xFFFFFFFFFFFFFFFF)
ROW_CAP = 2_000_000


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
    return nat.join_geometry()


class Joined:
    """t9_join_count on (lk, rk) with a 0xFF-filled workspace; emit(n_out)
    may be called repeatedly on it."""

    def __init__(self, nat, lk, rk):
        self.nat = nat
        self.lk = np.ascontiguousarray(lk, dtype=np.uint64)
        self.rk = np.ascontiguousarray(rk, dtype=np.uint64)
        self.nl, self.nr = len(self.lk), len(self.rk)
        self.d_lk = G.dev(self.lk) if self.nl else None
        self.d_rk = G.dev(self.rk) if self.nr else None
        self.ws = G.ws(nat.ws("join", self.nl, self.nr))
        self.ws.fill_(0xFF)
        self.total = nat.join_count(
            G.ptr(self.d_lk) if self.nl else None, self.nl,
            G.ptr(self.d_rk) if self.nr else None, self.nr,
            G.ptr(self.ws), G.stream())

    def emit(self, n_out, shift=0):
        """first min(n_out, total) result pairs; the guard words behind
        n_out (and the `shift` words in front of the outputs, which move
        them off their 16-byte alignment) must survive."""
        ol = G.dev(np.full(shift + n_out + NGUARD, GUARD, np.uint32))
        orr = G.dev(np.full(shift + n_out + NGUARD, GUARD, np.uint32))
        self.nat.join_emit(self.nl, self.nr, G.ptr(self.ws), n_out,
                           ol.data_ptr() + 4 * shift,
                           orr.data_ptr() + 4 * shift, G.stream())
        torch.cuda.synchronize()
        hl, hr = G.host(ol, np.uint32), G.host(orr, np.uint32)
        m = min(n_out, self.total)
        for h in (hl, hr):
            assert np.all(h[:shift] == GUARD), "wrote before the output"
            assert np.all(h[shift + m:] == GUARD), \
                "wrote at or past min(n_out, total)"
        return hl[shift:shift + m], hr[shift:shift + m]

    def inputs_unchanged(self):
        if self.nl:
            assert np.array_equal(G.host(self.d_lk, np.uint64), self.lk)
        if self.nr:
            assert np.array_equal(G.host(self.d_rk, np.uint64), self.rk)


def check(nat, lk, rk, expect_total=None):
    """full join of (lk, rk) equals the checker's; returns the Joined and
    the expected index arrays."""
    el, er = J.join(lk, rk)
    assert len(el) <= ROW_CAP
    if expect_total is not None:
        assert len(el) == expect_total, (len(el), expect_total)
    j = Joined(nat, lk, rk)
    assert j.total == len(el), (j.total, len(el))
    gl, gr = j.emit(j.total)
    assert np.array_equal(gl, el)
    assert np.array_equal(gr, er)
    j.inputs_unchanged()
    return j, el, er


def shuffled(a, seed):
    return np.random.default_rng(seed).permutation(
        np.asarray(a, dtype=np.uint64))


# ------------------------------------------------- reference-test shapes

def test_unique_keys_both_sides(nat):
    n = 9999
    check(nat, shuffled(np.arange(n), 1), shuffled(np.arange(n), 2), n)


@pytest.mark.parametrize("nl,nr", [(333, 333), (50, 333)])
def test_single_key(nat, nl, nr):
    check(nat, np.full(nl, 42, np.uint64), np.full(nr, 42, np.uint64),
          nl * nr)


def test_no_key_in_common(nat, geo):
    LT, OT, SK = geo
    n = LT + 17
    check(nat, shuffled(2 * np.arange(n), 3),
          shuffled(2 * np.arange(n) + 1, 4), 0)


def test_empty_sides(nat):
    for nl, nr in ((0, 0), (0, 5), (5, 0)):
        j = Joined(nat, np.arange(nl), np.arange(nr))
        assert j.total == 0
        gl, gr = j.emit(16)
        assert len(gl) == 0 and len(gr) == 0


# ------------------------------------------------------------------ keys

def test_keys_zero_and_all_ones(nat):
    rng = np.random.default_rng(5)
    lk = rng.integers(0, 1 << 63, 700, dtype=np.uint64) * np.uint64(2)
    rk = lk[rng.integers(0, 700, 500)].copy()
    lk[[3, 400, 401]] = 0
    lk[[7, 650]] = TOP
    rk[[0, 100]] = 0
    rk[[250, 251, 499]] = TOP
    j, el, er = check(nat, lk, rk)
    # six pairs on key 0 come first, six on 2^64-1 last
    assert np.all(lk[el[:6]] == 0) and np.all(rk[er[:6]] == 0)
    assert np.all(lk[el[-6:]] == TOP) and np.all(rk[er[-6:]] == TOP)


# -------------------------------------------------------- left-tile edges

def test_left_tile_edges(nat, geo):
    LT, OT, SK = geo
    rng = np.random.default_rng(6)
    rk = rng.integers(0, 3000, 2500, dtype=np.uint64)
    for nl in (1, LT - 1, LT, LT + 1, 2 * LT + 3):
        check(nat, rng.integers(0, 3000, nl, dtype=np.uint64), rk)


def test_equal_left_keys_straddle_a_tile(nat, geo):
    LT, OT, SK = geo
    # sorted left: LT-5 distinct keys, then 11 copies of one key across the
    # boundary at LT, then more distinct keys
    lk = np.concatenate([np.arange(LT - 5), np.full(11, LT + 100),
                         np.arange(LT + 200, LT + 300)])
    rk = np.concatenate([np.arange(0, LT + 300, 7), np.full(3, LT + 100)])
    check(nat, shuffled(lk, 7), shuffled(rk, 8))


# --------------------------------------------------------- stage overflow

@pytest.mark.parametrize("mul,add", [(1, 0), (1, 1), (4, 0)],
                         ids=["SK-lds", "SK+1-global", "4SK-global"])
def test_right_slice_vs_lds_stage(nat, geo, mul, add):
    LT, OT, SK = geo
    m = mul * SK + add
    # one left tile: its first key is below and its last above all m
    # distinct right keys 1..m; four left elements match
    lk = np.array([0, 5, 5, m // 2, m, m + 1], np.uint64)
    assert len(lk) <= LT
    check(nat, lk, shuffled(np.arange(1, m + 1), 9), 4)


def test_long_right_slice_with_duplicates(nat, geo):
    LT, OT, SK = geo
    m = SK + 300
    rk = np.concatenate([np.arange(1, m + 1), np.full(4, 77),
                         np.full(2, m)])
    lk = np.array([0, 77, 77, m, m + 1, 3], np.uint64)
    check(nat, shuffled(lk, 10), shuffled(rk, 11), 2 * 5 + 3 + 1)


# ------------------------------------------------------ output-tile edges

def test_totals_around_one_output_tile(nat, geo):
    LT, OT, SK = geo
    for n in (OT - 1, OT, OT + 1):
        check(nat, shuffled(np.arange(n), n), shuffled(np.arange(n), n + 1),
              n)


def test_tile_boundary_inside_a_group(nat, geo):
    LT, OT, SK = geo
    # three left elements of OT/2 + 7 rows each: the boundary at OT falls
    # inside the second group
    check(nat, np.full(3, 9, np.uint64), np.full(OT // 2 + 7, 9, np.uint64),
          3 * (OT // 2 + 7))


def test_tile_boundary_between_groups(nat, geo):
    LT, OT, SK = geo
    # two groups of OT/2 rows fill tile 0 exactly; position OT starts the
    # group of key 8
    lk = np.array([8, 3, 3], np.uint64)
    rk = np.concatenate([np.full(OT // 2, 3), np.full(5, 8)])
    check(nat, lk, shuffled(rk, 12), OT + 5)


def test_tile_starts_after_a_long_zero_count_run(nat, geo):
    LT, OT, SK = geo
    z = 2 * OT + 5
    # sorted left: key 0 (OT rows), z keys without a match, then the key
    # that owns the first row of tile 1
    lk = np.concatenate([[0], np.arange(1, z + 1), [z + 10, z + 10]])
    rk = np.concatenate([np.full(OT, 0), np.full(3, z + 10)])
    check(nat, shuffled(lk, 13), shuffled(rk, 14), OT + 6)


# ------------------------------------------------------------------- skew

def test_one_left_element_over_many_tiles(nat, geo):
    LT, OT, SK = geo
    n = 3 * OT + 1
    check(nat, np.array([5], np.uint64), np.full(n, 5, np.uint64), n)
    check(nat, np.full(n, 5, np.uint64), np.array([5], np.uint64), n)


def test_hot_key_amid_unique_keys(nat):
    hot = np.uint64(123456)
    lk = np.concatenate([np.arange(10_000) * 50, np.full(1000, hot)])
    rk = np.concatenate([np.arange(10_000) * 50, np.full(1000, hot)])
    check(nat, shuffled(lk, 15), shuffled(rk, 16), 10_000 + 1_000_000)


# ----------------------------------------------------------------- random

def test_random_many_to_many(nat):
    rng = np.random.default_rng(1)
    lk = rng.integers(0, 5000, 20_000, dtype=np.uint64)
    rk = rng.integers(0, 5000, 15_000, dtype=np.uint64)
    check(nat, lk, rk, 60_176)


def test_zipf_keys(nat):
    from thrill_amd.pipeline import zipf_cdf
    cdf = zipf_cdf(1000, 1.1)
    rng = np.random.default_rng(17)
    n = 20_000
    while True:
        lk = np.searchsorted(cdf, rng.random(n)).astype(np.uint64)
        rk = np.searchsorted(cdf, rng.random(n)).astype(np.uint64)
        if J.total(lk, rk) <= ROW_CAP:
            break
        n = n * 3 // 4
    assert n >= 1000
    check(nat, lk, rk)


# ------------------------------------------------------------ prefix emit

def test_prefix_emit_and_second_full_emit(nat, geo):
    LT, OT, SK = geo
    rng = np.random.default_rng(18)
    lk = rng.integers(0, 900, 3 * LT + 11, dtype=np.uint64)
    rk = rng.integers(0, 900, 1500, dtype=np.uint64)
    j, el, er = check(nat, lk, rk)
    assert j.total > 2 * OT
    for n_out in (j.total // 2, 0, OT + 1, j.total + 100):
        gl, gr = j.emit(n_out)
        m = min(n_out, j.total)
        assert np.array_equal(gl, el[:m]) and np.array_equal(gr, er[:m])
    gl, gr = j.emit(j.total)
    assert np.array_equal(gl, el) and np.array_equal(gr, er)
    j.inputs_unchanged()


# --------------------------------------------------------------- variants

def test_outputs_off_16_byte_alignment(nat, geo):
    LT, OT, SK = geo
    rng = np.random.default_rng(20)
    lk = rng.integers(0, 700, 2 * LT + 9, dtype=np.uint64)
    rk = rng.integers(0, 700, 1200, dtype=np.uint64)
    j, el, er = check(nat, lk, rk)
    for shift in (1, 2, 3):
        for n_out in (j.total, j.total - 3, OT + 2):
            gl, gr = j.emit(n_out, shift=shift)
            assert np.array_equal(gl, el[:n_out])
            assert np.array_equal(gr, er[:n_out])


@pytest.mark.parametrize("gallop,v4", [("0", "0"), ("0", "1"), ("1", "0")])
def test_kernel_variants_agree(nat, geo, monkeypatch, gallop, v4):
    # the defaults (both on) run everywhere else
    LT, OT, SK = geo
    monkeypatch.setenv("T9_JOIN_GALLOP", gallop)
    monkeypatch.setenv("T9_JOIN_EMIT_V4", v4)
    rng = np.random.default_rng(21)
    # many-to-many over two left tiles; runs of every length up to ~20
    j, el, er = check(nat, rng.integers(0, 500, 2 * LT + 3, dtype=np.uint64),
                      rng.integers(0, 500, 3000, dtype=np.uint64))
    for n_out in (j.total // 2 + 1, OT - 1, 0):
        gl, gr = j.emit(n_out)
        assert np.array_equal(gl, el[:n_out])
        assert np.array_equal(gr, er[:n_out])
    # a long run of equal right keys inside the LDS stage, unmatched keys
    rk = np.concatenate([np.full(SK // 2, 40), np.arange(100, 600)])
    check(nat, np.array([40, 39, 41, 40, 100, 599, 600], np.uint64),
          shuffled(rk, 22), 2 * (SK // 2) + 2)
    # a tile that starts after a long zero-count run
    z = 2 * OT + 5
    lk = np.concatenate([[0], np.arange(1, z + 1), [z + 10, z + 10]])
    rk = np.concatenate([np.full(OT, 0), np.full(3, z + 10)])
    check(nat, shuffled(lk, 13), shuffled(rk, 14), OT + 6)


# --------------------------------------------------------------- pipeline

def pipeline_inputs():
    rng = np.random.default_rng(19)
    lk = rng.integers(0, 2000, 7000, dtype=np.uint64)
    rk = rng.integers(0, 2000, 5000, dtype=np.uint64)
    lk[10] = rk[20] = TOP
    lv = rng.integers(0, 1 << 63, len(lk), dtype=np.uint64)
    rv = rng.integers(0, 1 << 63, len(rk), dtype=np.uint64)
    return lk, lv, rk, rv


def pipeline_step(lk, lv, rk, rv):
    from thrill_amd.pipeline import InnerJoin
    ij = InnerJoin(rank=0, world=1, device=0)
    d = [G.dev(a) for a in (lk, lv, rk, rv)]
    keys, lvals, rvals, m = ij.step(*d)
    torch.cuda.synchronize()
    out = [G.host(t, np.uint64) for t in (keys, lvals, rvals)]
    for t, a in zip(d, (lk, lv, rk, rv)):
        assert np.array_equal(G.host(t, np.uint64), a)
    ij.close()
    assert all(len(o) == m for o in out)
    return out


def test_pipeline_inner_join(nat):
    assert not os.environ.get("T9_FORCE_DIST")
    lk, lv, rk, rv = pipeline_inputs()
    el, er = J.join(lk, rk)
    keys, lvals, rvals = pipeline_step(lk, lv, rk, rv)
    assert np.array_equal(keys, lk[el])
    assert np.array_equal(lvals, lv[el])
    assert np.array_equal(rvals, rv[er])
    # an empty side joins to nothing
    e = np.zeros(0, np.uint64)
    assert all(len(o) == 0 for o in pipeline_step(e, e, rk, rv))


def test_pipeline_inner_join_distributed_branch_world1(nat):
    # hash partition -> exchange (loopback) -> local join: the stable
    # partition of one rank is the identity, so the tensors are identical
    import torch.distributed as dist
    lk, lv, rk, rv = pipeline_inputs()
    single = pipeline_step(lk, lv, rk, rv)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29561",
                            rank=0, world_size=1)
    old = os.environ.get("T9_FORCE_DIST")
    os.environ["T9_FORCE_DIST"] = "1"
    try:
        forced = pipeline_step(lk, lv, rk, rv)
    finally:
        if old is None:
            del os.environ["T9_FORCE_DIST"]
        else:
            os.environ["T9_FORCE_DIST"] = old
        dist.destroy_process_group()
    for a, b in zip(single, forced):
        assert np.array_equal(a, b)
