"""CPU-side checks of the join's C-ABI boundary: the four symbols load from
libt9.so with the header's arity, the geometry and workspace queries are
pure host code, every invalid call is refused with T9_EINVAL before any
device call, and an empty side is T9_OK with a zero total — so all of it
returns without a GPU."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "thrill_amd.h")
T9_SO = os.path.join(REPO, "thrill_amd", "libt9.so")

JOIN_SYMBOLS = ["t9_join_geometry", "t9_join_workspace", "t9_join_count",
                "t9_join_emit"]

OK, EINVAL = 0, -22
# never dereferenced: every call below must end during validation
FAKE = ctypes.c_void_p(0x1000)
SENTINEL = 0xDEADBEEF


@pytest.fixture(scope="module")
def t9lib():
    if not os.path.exists(T9_SO):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(REPO, "thrill_amd"),
                        "-j4"], check=True, capture_output=True)
    lib = ctypes.CDLL(T9_SO)
    from thrill_amd.native import _SIGS
    for s in JOIN_SYMBOLS:
        fn = getattr(lib, s)
        fn.restype, fn.argtypes = _SIGS[s]
    return lib


def geometry(lib):
    lt, ot, sk = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
    lib.t9_join_geometry(ctypes.byref(lt), ctypes.byref(ot),
                         ctypes.byref(sk))
    return lt.value, ot.value, sk.value


def count(lib, nl=16, nr=16, lkeys=FAKE, rkeys=FAKE, total="own", ws=FAKE):
    """(rc, *total); total="own" passes a word preset to SENTINEL."""
    t = ctypes.c_uint64(SENTINEL)
    tp = ctypes.byref(t) if total == "own" else total
    rc = lib.t9_join_count(None, lkeys, nl, rkeys, nr, tp, ws, None)
    return rc, t.value


def emit(lib, nl=16, nr=16, ws=FAKE, n_out=16, ol=FAKE, orr=FAKE):
    return lib.t9_join_emit(None, nl, nr, ws, n_out, ol, orr, None)


def test_symbols_exported_with_matching_arity(t9lib):
    from thrill_amd.native import _SIGS
    with open(HEADER) as f:
        text = f.read()
    for s in JOIN_SYMBOLS:
        assert hasattr(t9lib, s), f"libt9.so missing symbol {s}"
        m = re.search(r"^(?:int|uint64_t|void)\s+" + s + r"\s*\(([^)]*)\)",
                      text, re.M)
        assert m, f"{s} not declared in thrill_amd.h"
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        assert len(_SIGS[s][1]) == nargs, (s, len(_SIGS[s][1]), nargs)


def test_geometry_is_nonzero(t9lib):
    lt, ot, sk = geometry(t9lib)
    assert lt > 0 and ot > 0 and sk > 0
    # 256-thread blocks take whole rounds of a tile
    assert lt % 256 == 0 and ot % 256 == 0
    # NULL out-pointers are skipped, not written
    t9lib.t9_join_geometry(None, None, None)


def test_workspace_monotone_and_host_safe(t9lib):
    lt, ot, sk = geometry(t9lib)
    f = t9lib.t9_join_workspace
    ns = [0, 1, lt - 1, lt, lt + 1, 2 * lt + 3, sk + 1, 1 << 22, 1 << 26,
          (1 << 32) - 1]
    for m in (0, 1, 12345, 1 << 26):
        a = [f(n, m) for n in ns]
        b = [f(m, n) for n in ns]
        assert a == sorted(a), a
        assert b == sorted(b), b
    for n in ns:
        # sorted keys and indices of both sides, lo, cnt, off
        assert f(n, n) >= n * (8 + 4) * 2 + n * (4 + 8 + 8)
    assert f(0, 0) > 0


@pytest.mark.parametrize("big", [1 << 32, (1 << 32) + 1, 1 << 40])
def test_side_of_2_pow_32_or_more_is_refused(t9lib, big):
    assert count(t9lib, nl=big)[0] == EINVAL
    assert count(t9lib, nr=big)[0] == EINVAL
    assert count(t9lib, nl=big, nr=0)[0] == EINVAL
    assert emit(t9lib, nl=big) == EINVAL
    assert emit(t9lib, nr=big) == EINVAL


def test_null_pointers_are_refused(t9lib):
    assert count(t9lib, total=None)[0] == EINVAL
    assert count(t9lib, nl=0, nr=0, total=None)[0] == EINVAL
    assert count(t9lib, lkeys=None)[0] == EINVAL
    assert count(t9lib, rkeys=None)[0] == EINVAL
    assert count(t9lib, ws=None)[0] == EINVAL
    assert emit(t9lib, ws=None) == EINVAL
    assert emit(t9lib, ol=None) == EINVAL
    assert emit(t9lib, orr=None) == EINVAL


def test_misaligned_workspace_is_refused(t9lib):
    odd = ctypes.c_void_p(0x1008)
    assert count(t9lib, ws=odd)[0] == EINVAL
    assert emit(t9lib, ws=odd) == EINVAL


def test_a_refused_count_leaves_total_alone(t9lib):
    assert count(t9lib, lkeys=None) == (EINVAL, SENTINEL)
    assert count(t9lib, nl=1 << 32) == (EINVAL, SENTINEL)


@pytest.mark.parametrize("nl,nr", [(0, 0), (0, 16), (16, 0)])
def test_empty_side_is_ok_with_zero_total(t9lib, nl, nr):
    assert count(t9lib, nl=nl, nr=nr) == (OK, 0)
    # the keys of an empty side may be NULL
    assert count(t9lib, nl=nl, nr=nr, lkeys=None if nl == 0 else FAKE,
                 rkeys=None if nr == 0 else FAKE) == (OK, 0)
    # nothing to emit: no launch, whatever the buffers
    assert emit(t9lib, nl=nl, nr=nr) == OK


def test_emit_of_nothing_is_ok(t9lib):
    assert emit(t9lib, n_out=0) == OK
    assert emit(t9lib, n_out=0, ol=None, orr=None) == OK
