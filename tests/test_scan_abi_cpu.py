"""CPU-side checks of the scan family's C-ABI boundary: the five symbols
load from libt9.so with the header's arity, the geometry and workspace
queries are pure host code, and every invalid call is refused with
T9_EINVAL before any device call — so it returns without a GPU."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "thrill_amd.h")
T9_SO = os.path.join(REPO, "thrill_amd", "libt9.so")

SCAN_SYMBOLS = ["t9_scan_geometry", "t9_scan_workspace", "t9_scan_u64",
                "t9_scan_kv", "t9_fold_u64"]

OK, EINVAL = 0, -22
SUM, MIN, MAX = 0, 1, 2
U64, I64, F64 = 0, 1, 2
# never dereferenced: every call below must end during validation
FAKE = ctypes.c_void_p(0x1000)


@pytest.fixture(scope="module")
def t9lib():
    if not os.path.exists(T9_SO):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(REPO, "thrill_amd"),
                        "-j4"], check=True, capture_output=True)
    lib = ctypes.CDLL(T9_SO)
    from thrill_amd.native import _SIGS
    for s in SCAN_SYMBOLS:
        fn = getattr(lib, s)
        fn.restype, fn.argtypes = _SIGS[s]
    return lib


def scan_u64(lib, op=MAX, vtype=U64, n=16, excl=0, d_in=FAKE, d_out=FAKE,
             total=None, ws=FAKE):
    return lib.t9_scan_u64(None, d_in, d_out, n, op, vtype, excl, 0, total,
                           ws, None)


def scan_kv(lib, op=MAX, vtype=U64, n=16, d_in=FAKE, d_out=FAKE, total=None,
            ws=FAKE):
    return lib.t9_scan_kv(None, d_in, d_out, n, op, vtype, 0, total, ws,
                          None)


def fold(lib, op=MAX, vtype=U64, n=16, stride=1, d_in=FAKE, d_out=FAKE,
         ws=FAKE):
    return lib.t9_fold_u64(None, d_in, n, stride, op, vtype, d_out, ws,
                           None)


def test_symbols_exported_with_matching_arity(t9lib):
    from thrill_amd.native import _SIGS
    with open(HEADER) as f:
        text = f.read()
    for s in SCAN_SYMBOLS:
        assert hasattr(t9lib, s), f"libt9.so missing symbol {s}"
        m = re.search(r"^(?:int|uint64_t|void)\s+" + s + r"\s*\(([^)]*)\)",
                      text, re.M)
        assert m, f"{s} not declared in thrill_amd.h"
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        assert len(_SIGS[s][1]) == nargs, (s, len(_SIGS[s][1]), nargs)


def test_geometry_is_nonzero(t9lib):
    t, p = ctypes.c_uint32(0), ctypes.c_uint32(0)
    t9lib.t9_scan_geometry(ctypes.byref(t), ctypes.byref(p))
    assert t.value > 0 and p.value > 0
    # 16-byte accesses by 64-lane waves: a tile is whole wave accesses
    assert t.value % 128 == 0


def test_workspace_monotone_and_host_safe(t9lib):
    t, p = ctypes.c_uint32(0), ctypes.c_uint32(0)
    t9lib.t9_scan_geometry(ctypes.byref(t), ctypes.byref(p))
    T = t.value
    f = t9lib.t9_scan_workspace
    ns = [0, 1, T - 1, T, T + 1, 5 * T + 3, p.value * T, p.value * T + 1,
          1 << 28, 1 << 33, 1 << 40]
    sizes = [f(n) for n in ns]
    assert sizes == sorted(sizes), sizes
    for n, b in zip(ns, sizes):
        tiles = (n + T - 1) // T
        assert b >= 8 * tiles, (n, b)


@pytest.mark.parametrize("op,vtype", [(3, 0), (-1, 0), (1, 3), (1, -1),
                                      (99, 99)])
def test_out_of_range_op_or_vtype(t9lib, op, vtype):
    assert scan_u64(t9lib, op, vtype) == EINVAL
    assert scan_kv(t9lib, op, vtype) == EINVAL
    assert fold(t9lib, op, vtype) == EINVAL
    # refused even when there is nothing to do
    assert scan_u64(t9lib, op, vtype, n=0) == EINVAL
    assert fold(t9lib, op, vtype, n=0) == EINVAL


def test_f64_sum_is_refused(t9lib):
    assert scan_u64(t9lib, SUM, F64) == EINVAL
    assert scan_kv(t9lib, SUM, F64) == EINVAL
    assert fold(t9lib, SUM, F64) == EINVAL


@pytest.mark.parametrize("excl", [2, -1, 100])
def test_exclusive_must_be_0_or_1(t9lib, excl):
    assert scan_u64(t9lib, excl=excl) == EINVAL


@pytest.mark.parametrize("stride", [0, 3, 4, 16])
def test_stride_must_be_1_or_2(t9lib, stride):
    assert fold(t9lib, stride=stride) == EINVAL


def test_null_pointers_are_refused(t9lib):
    assert scan_u64(t9lib, d_in=None) == EINVAL
    assert scan_u64(t9lib, d_out=None) == EINVAL
    assert scan_u64(t9lib, ws=None) == EINVAL
    assert scan_kv(t9lib, d_in=None) == EINVAL
    assert scan_kv(t9lib, d_out=None) == EINVAL
    assert scan_kv(t9lib, ws=None) == EINVAL
    assert fold(t9lib, d_in=None) == EINVAL
    assert fold(t9lib, ws=None) == EINVAL
    assert fold(t9lib, d_out=None) == EINVAL
    # the fold's result pointer is needed even for n == 0
    assert fold(t9lib, n=0, d_out=None) == EINVAL


def test_too_many_tiles_is_refused(t9lib):
    t, p = ctypes.c_uint32(0), ctypes.c_uint32(0)
    t9lib.t9_scan_geometry(ctypes.byref(t), ctypes.byref(p))
    n = t.value << 31
    assert scan_u64(t9lib, n=n) == EINVAL
    assert scan_kv(t9lib, n=n) == EINVAL
    assert fold(t9lib, n=n) == EINVAL


@pytest.mark.parametrize("op,vtype", [(SUM, U64), (MIN, I64), (MAX, F64)])
def test_empty_scan_without_total_is_ok(t9lib, op, vtype):
    # nothing to write: T9_OK without touching the device, NULLs and all
    assert scan_u64(t9lib, op, vtype, n=0, d_in=None, d_out=None,
                    ws=None) == OK
    assert scan_u64(t9lib, op, vtype, n=0, excl=1) == OK
    assert scan_kv(t9lib, op, vtype, n=0, d_in=None, d_out=None,
                   ws=None) == OK
