"""bench.py command line: a plain run prints the headline line only and
--dump-outputs writes the last timed step's output (checked bit-exact
against the oracle at the sampled positions); --full adds the checks,
roofline, per-kernel breakdown and CPU baseline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 200_003
SEED = 0x99


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bench(*extra):
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--steps", "2", "--warmup", "1", "--records", str(N),
         "--seed", str(SEED)] + list(extra),
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_and_dump(tmp_path, oracle):
    out = tmp_path / "dump"
    res = _bench("--dump-outputs", str(out))
    assert res["steps"] == 2 and res["ms_per_step"] > 0
    assert res["unit"] == "keys/s" and res["higher_is_better"] is True
    assert res["dtype"] == "u8"
    # value = records / step time; ms_per_step is rounded to 0.01 ms
    assert abs(N / res["value"] * 1e3 - res["ms_per_step"]) <= 0.006
    for k in ("roofline", "cpu_baseline", "perf_breakdown", "validated"):
        assert res[k] is None, k

    files = sorted(p.name for p in out.iterdir())
    assert files == ["byte_column_sums.npy", "n_out.npy",
                     "records_sample.npy", "sample_positions.npy"]
    arrs = {f: np.load(out / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 * 2**20
    expect = oracle.sort_records(oracle.gen_records(N, seed=SEED))
    assert arrs["n_out.npy"].tolist() == [N]
    pos = arrs["sample_positions.npy"].astype(np.int64)
    assert pos[0] == 0 and pos[-1] == N - 1 and np.all(np.diff(pos) > 0)
    assert np.array_equal(arrs["records_sample.npy"],
                          expect[pos].astype(np.float32))
    assert np.array_equal(arrs["byte_column_sums.npy"],
                          expect.sum(axis=0, dtype=np.int64))


def test_full_run_reports_everything():
    res = _bench("--full")
    assert res["validated"] == {"keysum_conserved": True, "sorted": True}
    assert res["roofline"]["achieved"] > 0
    assert res["perf_breakdown"]["gather"]["launches"] >= 1
    assert res["cpu_baseline"]["value"] > 0
    assert res["ms_per_step"] > 0
