"""Run the compiled C++ join test binary (tests/cxx/join_test) on the GPU:
the four shapes of the reference's join test through t9::api::InnerJoin
(unique keys, one key on both sides, one key with different side sizes, two
item types), the deterministic output order, signed keys, empty and
disjoint sides; the binary itself proves through the "join_bounds" and
"join_emit" perf classes that the matching ran on the device. Built in-tree
by __graft_entry__.build()."""
import os
import subprocess

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "tests", "cxx", "join_test")


def test_join_cxx_surface():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if not os.path.exists(BIN):
        import __graft_entry__
        __graft_entry__.build()
    assert os.path.exists(BIN), "join_test binary missing"
    r = subprocess.run([BIN], cwd=REPO, capture_output=True, text=True,
                       timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
