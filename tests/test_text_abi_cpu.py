"""CPU-side checks of the text entry points' C-ABI boundary: every symbol
the header declares has a ctypes signature in thrill_amd.native, and the
tokenizer's workspace query is pure host code (no compute without a GPU)."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "thrill_amd.h")
T9_SO = os.path.join(REPO, "thrill_amd", "libt9.so")

TEXT_SYMBOLS = ["t9_text_tokenize_workspace", "t9_text_tokenize",
                "t9_text_hash2", "t9_reduce128_lookup",
                "t9_text_first_token"]


def declared_symbols():
    with open(HEADER) as f:
        text = f.read()
    return {m.group(1) for m in re.finditer(r"\b(t9_\w+)\s*\(", text)}


@pytest.fixture(scope="module")
def t9lib():
    if not os.path.exists(T9_SO):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(REPO, "thrill_amd"),
                        "-j4"], check=True, capture_output=True)
    return ctypes.CDLL(T9_SO)


def test_every_header_symbol_has_a_signature():
    from thrill_amd.native import _SIGS
    syms = declared_symbols()
    for s in TEXT_SYMBOLS:
        assert s in syms, f"{s} not declared in thrill_amd.h"
    missing = sorted(syms - set(_SIGS))
    assert not missing, f"no _SIGS entry for {missing}"


def test_text_symbols_exported_with_matching_arity(t9lib):
    from thrill_amd.native import _SIGS
    with open(HEADER) as f:
        text = f.read()
    for s in TEXT_SYMBOLS:
        assert hasattr(t9lib, s), f"libt9.so missing symbol {s}"
        m = re.search(r"^(?:int|uint64_t)\s+" + s + r"\s*\(([^)]*)\)", text,
                      re.M)
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        sig_args = len(_SIGS[s][1])
        assert sig_args == nargs, (s, sig_args, nargs)


def test_tokenize_workspace_host_safe(t9lib):
    f = t9lib.t9_text_tokenize_workspace
    f.restype = ctypes.c_uint64
    f.argtypes = [ctypes.c_uint64]
    sizes = [f(n) for n in (0, 1, 1 << 20, (1 << 32) - 1)]
    assert all(b > 0 for b in sizes), sizes
    assert sizes == sorted(sizes), sizes
