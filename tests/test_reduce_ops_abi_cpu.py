"""CPU-side checks of the reduce-operator entry points' C-ABI boundary: the
new symbols load from libt9.so with matching arity, the by-index workspace
query is pure host code, and an invalid call is refused with T9_EINVAL
before any device call — so it returns without a GPU."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "thrill_amd.h")
T9_SO = os.path.join(REPO, "thrill_amd", "libt9.so")

OP_SYMBOLS = ["t9_reduce_init_op", "t9_reduce_build_op",
              "t9_reduce_drain_op", "t9_reduce128_init_op",
              "t9_reduce128_build_op", "t9_reduce128_drain_op",
              "t9_reduce_by_index_op_workspace", "t9_reduce_by_index_op"]

EINVAL = -22
# never dereferenced: every call below must be refused during validation
FAKE = ctypes.c_void_p(0x1000)


@pytest.fixture(scope="module")
def t9lib():
    if not os.path.exists(T9_SO):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(REPO, "thrill_amd"),
                        "-j4"], check=True, capture_output=True)
    lib = ctypes.CDLL(T9_SO)
    from thrill_amd.native import _SIGS
    for s in OP_SYMBOLS:
        fn = getattr(lib, s)
        fn.restype, fn.argtypes = _SIGS[s]
    return lib


def test_enum_values_match_header():
    import thrill_amd
    from thrill_amd import native
    with open(HEADER) as f:
        text = f.read()
    for name in ("T9_OP_SUM", "T9_OP_MIN", "T9_OP_MAX", "T9_VAL_U64",
                 "T9_VAL_I64", "T9_VAL_F64"):
        m = re.search(name + r"\s*=\s*(\d+)", text)
        assert m, f"{name} not in thrill_amd.h"
        assert getattr(native, name) == int(m.group(1))
        assert getattr(thrill_amd, name) == int(m.group(1))


def test_op_symbols_exported_with_matching_arity(t9lib):
    from thrill_amd.native import _SIGS
    with open(HEADER) as f:
        text = f.read()
    for s in OP_SYMBOLS:
        assert hasattr(t9lib, s), f"libt9.so missing symbol {s}"
        m = re.search(r"^(?:int|uint64_t)\s+" + s + r"\s*\(([^)]*)\)", text,
                      re.M)
        assert m, f"{s} not declared in thrill_amd.h"
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        assert len(_SIGS[s][1]) == nargs, (s, len(_SIGS[s][1]), nargs)


def test_by_index_workspace_host_safe(t9lib):
    f = t9lib.t9_reduce_by_index_op_workspace
    sizes = [f(n) for n in (1, 31, 32, 33, 5000, 1 << 30)]
    # one bit per index at least
    for n, b in zip((1, 31, 32, 33, 5000, 1 << 30), sizes):
        assert b * 8 >= n, (n, b)
    assert sizes == sorted(sizes), sizes


def build_op(lib, op, vtype, cap=1024, keys=FAKE, vals=FAKE):
    return lib.t9_reduce_build_op(None, keys, vals, 16, FAKE, cap, 0, op,
                                  vtype, FAKE, None)


def test_f64_sum_is_refused(t9lib):
    from thrill_amd.native import T9_OP_SUM, T9_VAL_F64
    assert build_op(t9lib, T9_OP_SUM, T9_VAL_F64) == EINVAL
    assert t9lib.t9_reduce_init_op(None, FAKE, 1024, T9_OP_SUM, T9_VAL_F64,
                                   None) == EINVAL
    assert t9lib.t9_reduce_by_index_op(
        None, FAKE, FAKE, 16, 0, 64, T9_OP_SUM, T9_VAL_F64, 0, FAKE, FAKE,
        FAKE, None) == EINVAL


@pytest.mark.parametrize("op,vtype", [(3, 0), (-1, 0), (1, 3), (1, -1),
                                      (99, 99)])
def test_out_of_range_op_or_vtype(t9lib, op, vtype):
    assert build_op(t9lib, op, vtype) == EINVAL
    assert t9lib.t9_reduce_init_op(None, FAKE, 1024, op, vtype,
                                   None) == EINVAL
    assert t9lib.t9_reduce_drain_op(None, FAKE, 1024, op, vtype, FAKE, FAKE,
                                    FAKE, None) == EINVAL
    assert t9lib.t9_reduce128_init_op(None, FAKE, 1024, op, vtype,
                                      None) == EINVAL
    assert t9lib.t9_reduce128_build_op(None, FAKE, FAKE, FAKE, 16, FAKE,
                                       1024, 0, op, vtype, FAKE,
                                       None) == EINVAL
    assert t9lib.t9_reduce128_drain_op(None, FAKE, 1024, op, vtype, FAKE,
                                       FAKE, FAKE, FAKE, None) == EINVAL
    assert t9lib.t9_reduce_by_index_op(
        None, FAKE, FAKE, 16, 0, 64, op, vtype, 0, FAKE, FAKE, FAKE,
        None) == EINVAL


def test_reduce128_count_one_needs_sum(t9lib):
    from thrill_amd.native import T9_OP_MAX, T9_OP_MIN, T9_VAL_U64
    for op in (T9_OP_MIN, T9_OP_MAX):
        assert t9lib.t9_reduce128_build_op(
            None, FAKE, FAKE, None, 16, FAKE, 1024, 0, op, T9_VAL_U64, FAKE,
            None) == EINVAL


@pytest.mark.parametrize("cap", [0, 3, 1000, (1 << 20) + 1])
def test_capacity_must_be_a_power_of_two(t9lib, cap):
    from thrill_amd.native import T9_OP_MIN, T9_VAL_I64
    op, vt = T9_OP_MIN, T9_VAL_I64
    assert build_op(t9lib, op, vt, cap=cap) == EINVAL
    assert t9lib.t9_reduce_init_op(None, FAKE, cap, op, vt, None) == EINVAL
    assert t9lib.t9_reduce_drain_op(None, FAKE, cap, op, vt, FAKE, FAKE,
                                    FAKE, None) == EINVAL
    assert t9lib.t9_reduce128_init_op(None, FAKE, cap, op, vt,
                                      None) == EINVAL
    assert t9lib.t9_reduce128_build_op(None, FAKE, FAKE, FAKE, 16, FAKE,
                                       cap, 0, op, vt, FAKE, None) == EINVAL
    assert t9lib.t9_reduce128_drain_op(None, FAKE, cap, op, vt, FAKE, FAKE,
                                       FAKE, FAKE, None) == EINVAL


def test_null_pointers_are_refused(t9lib):
    from thrill_amd.native import T9_OP_MAX, T9_VAL_U64
    op, vt = T9_OP_MAX, T9_VAL_U64
    assert build_op(t9lib, op, vt, keys=None) == EINVAL
    assert build_op(t9lib, op, vt, vals=None) == EINVAL
    assert t9lib.t9_reduce_init_op(None, None, 1024, op, vt, None) == EINVAL
    assert t9lib.t9_reduce_by_index_op(
        None, FAKE, FAKE, 16, 0, 64, op, vt, 0, FAKE, FAKE, None,
        None) == EINVAL
    assert t9lib.t9_reduce_by_index_op(
        None, FAKE, FAKE, 16, 0, 0, op, vt, 0, FAKE, FAKE, FAKE,
        None) == EINVAL


def test_stride4_is_refused_on_the_op_path(t9lib, monkeypatch):
    from thrill_amd.native import T9_OP_MIN, T9_VAL_U64
    monkeypatch.setenv("T9_R128_STRIDE", "4")
    assert t9lib.t9_reduce128_init_op(None, FAKE, 1024, T9_OP_MIN,
                                      T9_VAL_U64, None) == EINVAL
    assert t9lib.t9_reduce128_build_op(None, FAKE, FAKE, FAKE, 16, FAKE,
                                       1024, 0, T9_OP_MIN, T9_VAL_U64, FAKE,
                                       None) == EINVAL
    assert t9lib.t9_reduce128_drain_op(None, FAKE, 1024, T9_OP_MIN,
                                       T9_VAL_U64, FAKE, FAKE, FAKE, FAKE,
                                       None) == EINVAL
