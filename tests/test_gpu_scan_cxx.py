"""Run the compiled C++ scan-family test binary (tests/cxx/scan_test) on the
GPU: PrefixSum / ExPrefixSum with the reference's known answers, signed
min, double max, the KeyValue max-scan idiom, and the Sum / Min / Max /
AllReduce actions; the binary itself proves through the "scan" perf class
which cases ran on the device. Built in-tree by __graft_entry__.build()."""
import os
import subprocess

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "tests", "cxx", "scan_test")


def test_scan_cxx_surface():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if not os.path.exists(BIN):
        import __graft_entry__
        __graft_entry__.build()
    assert os.path.exists(BIN), "scan_test binary missing"
    r = subprocess.run([BIN], cwd=REPO, capture_output=True, text=True,
                       timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
