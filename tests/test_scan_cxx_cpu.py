"""CPU-side compile check of the scan family's C++ surface (hipcc
-fsyntax-only builds the test TU without a GPU): PrefixSum, ExPrefixSum,
Sum, Min, Max and AllReduce must instantiate for u64, i64, double and
KeyValue items, the default functor included."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_surface_compiles():
    r = subprocess.run(
        ["hipcc", "-O0", "-std=c++17", "-fsyntax-only",
         "-I" + os.path.join(REPO, "include"),
         os.path.join(REPO, "tests", "cxx", "scan_test.cpp")],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
