"""GPU parity tests for the wave-private form of the fused extract + pass-1
histogram (k_extract_hist_wave, T9_EXTRACT_WAVE): the keys, the index iota
and the per-tile top-byte histogram against numpy through the stand-alone
entry t9_extract_key64_hist, and against the block-staged form
(T9_EXTRACT_WAVE=0) on the same device input; then record sorts through it
against the CPU oracle / numpy and against the block-staged run.

Shapes sit on the edges of the structure: the 64-record wave sub-tile, the
2048-record wave quarter and the 8192-record tile. All comparisons are
exact (integer and byte work)."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tests import _gpu as G
    from thrill_amd import Native

TILE = 8192
WAVE_FORM = "1"      # T9_EXTRACT_WAVE value of the form under test
BLOCK_FORM = "0"     # the block-staged k_extract_hist
GUARD = 64           # untouched elements checked behind every output

SHAPES = [1, 63, 64, 65, 2047, 2048, 2049, 6145, 8191, 8192, 8193,
          3 * TILE + 2048 + 65]


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = Native(device=0)
    yield n
    n.close()


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def make_records(n, rec, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, rec), dtype=np.uint8)


def reference(recs, le):
    """(keys, iota, hist) the fused pass must produce."""
    n = recs.shape[0]
    keys = recs[:, :8].copy().view("<u8" if le else ">u8").reshape(-1) \
        .astype(np.uint64)
    top = (keys >> np.uint64(56)).astype(np.int64)
    tiles = -(-n // TILE)
    hist = np.zeros((tiles, 256), dtype=np.uint32)
    for t in range(tiles):
        hist[t] = np.bincount(top[t * TILE:(t + 1) * TILE], minlength=256)
    return keys, np.arange(n, dtype=np.uint32), hist.reshape(-1)


def run_extract(nat, rec_ptr, n, rec, le, widx, form):
    """One t9_extract_key64_hist call under T9_EXTRACT_WAVE=form; returns
    (keys, idx or None, hist) and asserts that nothing behind the n-th
    element of any output was written."""
    tiles = -(-n // TILE)
    dk = G.dev(np.full(n + GUARD, 0xA5A5A5A5A5A5A5A5, np.uint64))
    di = G.dev(np.full(n + GUARD, 0x5A5A5A5A, np.uint32))
    dh = G.dev(np.full(tiles * 256 + GUARD, 0xC3C3C3C3, np.uint32))
    with env(T9_EXTRACT_WAVE=form):
        nat.extract_key64_hist(rec_ptr, n, rec, 1 if le else 0, G.ptr(dk),
                               G.ptr(di) if widx else None, G.ptr(dh),
                               G.stream())
    torch.cuda.synchronize()
    hk, hi, hh = (G.host(dk, np.uint64), G.host(di, np.uint32),
                  G.host(dh, np.uint32))
    assert (hk[n:] == np.uint64(0xA5A5A5A5A5A5A5A5)).all(), \
        "keys written past n"
    assert (hh[tiles * 256:] == 0xC3C3C3C3).all(), "hist written past end"
    if widx:
        assert (hi[n:] == 0x5A5A5A5A).all(), "idx written past n"
    else:
        assert (hi == 0x5A5A5A5A).all(), "idx written though not asked for"
    return hk[:n], (hi[:n] if widx else None), hh[:tiles * 256]


def check_direct(nat, recs, rec_ptr, le, widx):
    n, rec = recs.shape
    ek, ei, eh = reference(recs, le)
    wk, wi, wh = run_extract(nat, rec_ptr, n, rec, le, widx, WAVE_FORM)
    bk, bi, bh = run_extract(nat, rec_ptr, n, rec, le, widx, BLOCK_FORM)
    assert np.array_equal(wk, ek), "wave form: keys"
    assert np.array_equal(wh, eh), "wave form: histogram"
    assert int(wh.sum()) == n
    assert np.array_equal(bk, ek), "block form: keys"
    assert np.array_equal(bh, eh), "block form: histogram"
    assert np.array_equal(wk, bk) and np.array_equal(wh, bh)
    if widx:
        assert np.array_equal(wi, ei), "wave form: iota"
        assert np.array_equal(bi, ei), "block form: iota"


# ------------------------------------------------------------ direct tests

@pytest.mark.parametrize("widx", [False, True], ids=["noidx", "idx"])
@pytest.mark.parametrize("rec,le", [(100, False), (128, True)],
                         ids=["be100", "le128"])
@pytest.mark.parametrize("n", SHAPES)
def test_extract_hist_edges(nat, n, rec, le, widx):
    recs = make_records(n, rec, seed=1000 + n + rec)
    d = G.dev(recs.reshape(-1))
    check_direct(nat, recs, G.ptr(d), le, widx)


def test_extract_hist_base_offset_by_4_bytes(nat):
    # the record base sits 4 bytes into a larger allocation: the entry
    # takes any 4-byte-aligned pointer, so no load may assume more
    n, rec = 3 * TILE + 2048 + 65, 100
    recs = make_records(n, rec, seed=4)
    buf = np.zeros(n * rec + 32, dtype=np.uint8)
    buf[4:4 + n * rec] = recs.reshape(-1)
    d = G.dev(buf)
    assert d.data_ptr() % 16 == 0
    check_direct(nat, recs, ctypes.c_void_p(d.data_ptr() + 4), False, True)


@pytest.mark.parametrize("rec,le", [(100, False), (128, True)],
                         ids=["be100", "le128"])
def test_extract_hist_one_top_byte(nat, rec, le):
    # every key has the same top byte: the ballot combine's degenerate
    # case, one LDS add of 64 per wave sub-tile
    n = TILE + 2048 + 65
    recs = make_records(n, rec, seed=7)
    recs[:, 7 if le else 0] = 0xAB
    d = G.dev(recs.reshape(-1))
    check_direct(nat, recs, G.ptr(d), le, False)
    _, _, eh = reference(recs, le)
    assert eh.reshape(-1, 256)[:, 0xAB].tolist() == [TILE, 2048 + 65]


def test_extract_hist_rejects_other_record_sizes(nat):
    from thrill_amd import T9Error
    d = G.dev(np.zeros(64 * 104, np.uint8))
    dk, dh = G.empty(64, np.uint64), G.empty(256, np.uint32)
    with pytest.raises(T9Error):
        nat.extract_key64_hist(G.ptr(d), 64, 104, 0, G.ptr(dk), None,
                               G.ptr(dh), G.stream())


# ------------------------------------------------------------- end to end

def sort_records(nat, recs, **extra):
    n, rec = recs.shape
    din = G.dev(recs.reshape(-1))
    dout = G.empty(n * rec, np.uint8)
    w = G.ws(nat.ws("sort_records", n, rec))
    outs = []
    for form in (WAVE_FORM, BLOCK_FORM):
        with env(T9_SORT_ALGO="msb", T9_EXTRACT_WAVE=form, **extra):
            if rec == 100:
                nat.sort_records(G.ptr(din), G.ptr(dout), n, rec, 10,
                                 G.ptr(w), G.stream())
            else:
                nat.sort_records_keyle(G.ptr(din), G.ptr(dout), n, rec,
                                       G.ptr(w), G.stream())
        outs.append(G.host(dout, np.uint8).reshape(n, rec).copy())
    return outs


@pytest.mark.parametrize("n", [16384, 16385, 16384 + 2049, 3 * TILE - 1])
def test_sort_records_through_wave_extract(nat, oracle, n):
    recs = oracle.gen_records(n, seed=300 + n)
    wave, block = sort_records(nat, recs)
    assert np.array_equal(wave, oracle.sort_records(recs))
    assert np.array_equal(wave, block)


def test_sort_records_through_wave_extract_with_iota(nat, oracle):
    n = 16384 + 2049
    recs = oracle.gen_records(n, seed=55)
    wave, block = sort_records(nat, recs, T9_EXTRACT_IOTA="1")
    assert np.array_equal(wave, oracle.sort_records(recs))
    assert np.array_equal(wave, block)


def test_sort_records_keyle_through_wave_extract(nat):
    n = 16384 + 65
    recs = make_records(n, 128, seed=91)
    recs[: n // 20, :8] = recs[0, :8]   # duplicate numeric keys
    wave, block = sort_records(nat, recs)
    keys = recs[:, :8].copy().view("<u8").reshape(-1)
    order = np.lexsort(tuple(recs[:, c] for c in range(127, 7, -1))
                       + (keys,))
    assert np.array_equal(wave, recs[order])
    assert np.array_equal(wave, block)
