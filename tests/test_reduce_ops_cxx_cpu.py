"""CPU-side compile check of the reduce-operator C++ surface (hipcc
-fsyntax-only builds the test TU without a GPU): the ReducePair overload
with a reduce function, ReduceToIndex and the ReduceByKey min/max branch
must instantiate."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reduce_op_surface_compiles():
    r = subprocess.run(
        ["hipcc", "-O0", "-std=c++17", "-fsyntax-only",
         "-I" + os.path.join(REPO, "include"),
         os.path.join(REPO, "tests", "cxx", "reduce_op_test.cpp")],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
