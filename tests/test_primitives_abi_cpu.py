"""CPU-side checks of the C-ABI boundary of the sort and reduce support
primitives (classify, partition, bucket mappings, reduce-by-index, merge,
gather, extract, group index): every invalid call below is refused with
T9_EINVAL, and every empty merge answered with T9_OK, before any device
call — so each returns without a GPU. The workspace queries are pure host
code. So are the 128-bit reduce table's sizing query and the refusal of a
4-word slot stride by a build variant that has none."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T9_SO = os.path.join(REPO, "thrill_amd", "libt9.so")
HEADER = os.path.join(REPO, "include", "thrill_amd.h")

SYMBOLS = ["t9_classify_u64", "t9_classify_rec", "t9_partition_idx",
           "t9_partition_idx_workspace", "t9_hash_bucket", "t9_bucket_mod",
           "t9_index_bucket", "t9_reduce_by_index", "t9_merge_u64",
           "t9_merge_records", "t9_gather_records", "t9_extract_key64",
           "t9_extract_key64_le", "t9_group_index",
           "t9_group_index_workspace", "t9_reduce128_table_words",
           "t9_reduce128_init", "t9_reduce128_build", "t9_reduce128_drain",
           "t9_reduce128_lookup"]

OK, EINVAL = 0, -22
# never dereferenced: every call below must end during validation
FAKE = ctypes.c_void_p(0x1000)
BAD_P = [0, 257, 1 << 31]


@pytest.fixture(scope="module")
def t9lib():
    if not os.path.exists(T9_SO):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(REPO, "thrill_amd"),
                        "-j4"], check=True, capture_output=True)
    lib = ctypes.CDLL(T9_SO)
    from thrill_amd.native import _SIGS
    for s in SYMBOLS:
        fn = getattr(lib, s)
        fn.restype, fn.argtypes = _SIGS[s]
    return lib


def classify_u64(lib, p=8, n=16, counts=FAKE):
    return lib.t9_classify_u64(None, FAKE, n, 0, FAKE, FAKE, p, FAKE,
                               counts, None)


def classify_rec(lib, p=8, n=16, rec=100, counts=FAKE):
    return lib.t9_classify_rec(None, FAKE, FAKE, n, 0, FAKE, FAKE, FAKE, p,
                               rec, FAKE, counts, None)


def partition_idx(lib, p=8, n=16, offsets=FAKE):
    return lib.t9_partition_idx(None, FAKE, n, p, FAKE, offsets, FAKE, None)


def hash_bucket(lib, p=8, n=16, counts=FAKE):
    return lib.t9_hash_bucket(None, FAKE, n, 0, p, FAKE, counts, None)


def bucket_mod(lib, p=8, n=16, counts=FAKE):
    return lib.t9_bucket_mod(None, FAKE, n, p, FAKE, counts, None)


def index_bucket(lib, p=8, n=16, size=100, counts=FAKE, error=FAKE):
    return lib.t9_index_bucket(None, FAKE, n, 0, size, p, FAKE, counts,
                               error, None)


def reduce_by_index(lib, n=16, size=100, dense=FAKE, error=FAKE):
    return lib.t9_reduce_by_index(None, FAKE, FAKE, n, 0, size, dense,
                                  error, None)


@pytest.mark.parametrize("p", BAD_P)
def test_partition_count_outside_1_to_256_is_refused(t9lib, p):
    for call in (classify_u64, classify_rec, partition_idx, hash_bucket,
                 bucket_mod, index_bucket):
        assert call(t9lib, p=p) == EINVAL, call.__name__
        # refused even when there is nothing to do
        assert call(t9lib, p=p, n=0) == EINVAL, call.__name__


def test_null_result_pointers_are_refused(t9lib):
    for call in (classify_u64, classify_rec, hash_bucket, bucket_mod,
                 index_bucket):
        assert call(t9lib, counts=None) == EINVAL, call.__name__
        assert call(t9lib, counts=None, n=0) == EINVAL, call.__name__
    assert partition_idx(t9lib, offsets=None) == EINVAL
    assert partition_idx(t9lib, offsets=None, n=0) == EINVAL
    assert index_bucket(t9lib, error=None) == EINVAL
    assert reduce_by_index(t9lib, error=None) == EINVAL
    assert reduce_by_index(t9lib, dense=None) == EINVAL
    assert reduce_by_index(t9lib, dense=None, n=0) == EINVAL
    # the group count is needed even for n == 0
    for n in (0, 16):
        assert t9lib.t9_group_index(None, FAKE, n, FAKE, FAKE, None, FAKE,
                                    None) == EINVAL


@pytest.mark.parametrize("n", [0, 16])
def test_empty_index_range_is_refused(t9lib, n):
    assert reduce_by_index(t9lib, n=n, size=0) == EINVAL
    assert index_bucket(t9lib, n=n, size=0) == EINVAL


@pytest.mark.parametrize("rec", [0, 1, 2, 3, 6, 99, 101])
def test_record_size_must_be_a_positive_multiple_of_4(t9lib, rec):
    for n in (0, 16):
        assert t9lib.t9_merge_records(None, FAKE, n, FAKE, n, rec, FAKE,
                                      None) == EINVAL
        assert t9lib.t9_gather_records(None, FAKE, FAKE, n, rec, FAKE,
                                       None) == EINVAL


@pytest.mark.parametrize("rec", [0, 4, 7])
def test_classify_rec_needs_the_8_byte_prefix(t9lib, rec):
    assert classify_rec(t9lib, rec=rec) == EINVAL
    assert classify_rec(t9lib, rec=rec, n=0) == EINVAL


@pytest.mark.parametrize("rec,key_off", [
    (100, 96), (100, 100), (8, 4), (4, 0), (0, 0),   # key runs past the end
    (100, 1), (100, 2), (100, 6), (128, 7),          # key_off % 4
    (10, 0), (102, 4)])                              # rec_size % 4
def test_extract_key_window_is_validated(t9lib, rec, key_off):
    for fn in (t9lib.t9_extract_key64, t9lib.t9_extract_key64_le):
        for n in (0, 16):
            assert fn(None, FAKE, n, rec, key_off, FAKE, FAKE,
                      None) == EINVAL


def test_extract_and_gather_null_pointers_are_refused(t9lib):
    for fn in (t9lib.t9_extract_key64, t9lib.t9_extract_key64_le):
        assert fn(None, None, 16, 100, 0, FAKE, FAKE, None) == EINVAL
        assert fn(None, FAKE, 16, 100, 0, None, FAKE, None) == EINVAL
        assert fn(None, FAKE, 16, 100, 0, FAKE, None, None) == EINVAL
    g = t9lib.t9_gather_records
    assert g(None, None, FAKE, 16, 100, FAKE, None) == EINVAL
    assert g(None, FAKE, None, 16, 100, FAKE, None) == EINVAL
    assert g(None, FAKE, FAKE, 16, 100, None, None) == EINVAL


@pytest.mark.parametrize("n", [1 << 32, (1 << 32) + 1, 1 << 40])
def test_partition_idx_refuses_2_to_the_32_items(t9lib, n):
    assert partition_idx(t9lib, n=n) == EINVAL


def test_empty_merges_are_ok_without_touching_anything(t9lib):
    assert t9lib.t9_merge_u64(None, None, 0, None, 0, None, None) == OK
    assert t9lib.t9_merge_u64(None, FAKE, 0, FAKE, 0, FAKE, None) == OK
    for rec in (4, 8, 100, 128):
        assert t9lib.t9_merge_records(None, None, 0, None, 0, rec, None,
                                      None) == OK
        assert t9lib.t9_merge_records(None, FAKE, 0, FAKE, 0, rec, FAKE,
                                      None) == OK


@pytest.mark.parametrize("na,nb", [(1, 0), (0, 1), (1, 1), (5000, 3)])
def test_merge_without_an_output_is_refused(t9lib, na, nb):
    assert t9lib.t9_merge_u64(None, FAKE, na, FAKE, nb, None,
                              None) == EINVAL
    assert t9lib.t9_merge_records(None, FAKE, na, FAKE, nb, 100, None,
                                  None) == EINVAL


def test_merge_without_a_needed_input_is_refused(t9lib):
    assert t9lib.t9_merge_u64(None, None, 3, FAKE, 4, FAKE, None) == EINVAL
    assert t9lib.t9_merge_u64(None, FAKE, 3, None, 4, FAKE, None) == EINVAL
    assert t9lib.t9_merge_records(None, None, 3, FAKE, 4, 12, FAKE,
                                  None) == EINVAL
    assert t9lib.t9_merge_records(None, FAKE, 3, None, 4, 12, FAKE,
                                  None) == EINVAL


@pytest.mark.parametrize("query,tile,row_bytes", [
    ("t9_partition_idx_workspace", 2048, 1024),   # one 256-bin u32 hist row
    ("t9_group_index_workspace", 8192, 4)])       # one u32 block sum
def test_workspace_queries_are_monotone_and_nonzero(t9lib, query, tile,
                                                    row_bytes):
    f = getattr(t9lib, query)
    ns = [0, 1, 255, 256, 257, tile - 1, tile, tile + 1, 32 * tile,
          32 * tile + 1, 257 * tile + 3, 1 << 28, (1 << 32) - 1]
    sizes = [f(n) for n in ns]
    assert sizes[0] > 0
    assert sizes == sorted(sizes), sizes
    for n, b in zip(ns, sizes):
        assert b >= row_bytes * ((n + tile - 1) // tile), (n, b)


# ------------------------------------------------ 128-bit table slot stride

def test_reduce128_symbols_exported_with_matching_arity(t9lib):
    from thrill_amd.native import _SIGS
    with open(HEADER) as f:
        text = f.read()
    for s in SYMBOLS[-5:]:
        assert s.startswith("t9_reduce128_")
        assert hasattr(t9lib, s), f"libt9.so missing symbol {s}"
        m = re.search(r"^(?:int|uint64_t)\s+" + s + r"\s*\(([^)]*)\)", text,
                      re.M)
        assert m, f"{s} not declared in thrill_amd.h"
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        assert len(_SIGS[s][1]) == nargs, (s, len(_SIGS[s][1]), nargs)


def build128(lib, n=16, vals=FAKE):
    return lib.t9_reduce128_build(None, FAKE, FAKE, vals, n, FAKE, 1024, 0,
                                  FAKE, None)


@pytest.mark.parametrize("env", [
    {"T9_R128_READFIRST": "0"},
    {"T9_LDS128_SLOTS": "1024"},
    {"T9_LDS128_SLOTS": "2048"},
    {"T9_LDS128_SLOTS": "4095"},
    {"T9_LDS128_SLOTS": "2048", "T9_R128_READFIRST": "0"}],
    ids=lambda e: ",".join(f"{k[3:]}={v}" for k, v in e.items()))
def test_stride4_without_a_stride4_build_is_refused(t9lib, monkeypatch,
                                                    env):
    # init, drain and lookup would address 4-word slots; the selected build
    # variant exists with 3-word slots only: T9_EINVAL before any device
    # call, whatever n and vals are
    for k in ("T9_R128_READFIRST", "T9_LDS128_SLOTS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("T9_R128_STRIDE", "4")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert build128(t9lib) == EINVAL
    assert build128(t9lib, vals=None) == EINVAL
    assert build128(t9lib, n=0) == EINVAL


def test_reduce128_table_words_follows_the_stride_knob(t9lib, monkeypatch):
    f = t9lib.t9_reduce128_table_words
    caps = [1, 2, 16, 1024, 1 << 31]
    monkeypatch.delenv("T9_R128_STRIDE", raising=False)
    assert [f(c) for c in caps] == [3 * c for c in caps]
    monkeypatch.setenv("T9_R128_STRIDE", "4")
    assert [f(c) for c in caps] == [4 * c for c in caps]
    # any other value is the packed layout, as in init/build/drain/lookup
    for other in ("3", "0", "8", ""):
        monkeypatch.setenv("T9_R128_STRIDE", other)
        assert [f(c) for c in caps] == [3 * c for c in caps]
