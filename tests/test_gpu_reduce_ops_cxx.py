"""Run the compiled C++ reduce-operator test binary
(tests/cxx/reduce_op_test) on the GPU: ReducePair with a reduce function,
ReduceByKey with min/max on a signed counter, ReduceToIndex with a neutral
element. The binary is built in-tree by __graft_entry__.build()."""
import os
import subprocess

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "tests", "cxx", "reduce_op_test")


def test_reduce_op_cxx_surface():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if not os.path.exists(BIN):
        import __graft_entry__
        __graft_entry__.build()
    assert os.path.exists(BIN), "reduce_op_test binary missing"
    r = subprocess.run([BIN], cwd=REPO, capture_output=True, text=True,
                       timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
