"""Multi-process (gloo, world 3) CPU test of the distributed PrefixSum
protocol of thrill_amd/pipeline.py — fold the shard, all-gather the
per-rank totals, scan_carry, scan the shard from that carry — with numpy
as the compute, so the protocol (carry arithmetic in the encoded domain,
empty shards, rank order) is covered without a GPU. The concatenation of
the ranks' outputs must equal the scan of the whole array."""
import os

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import _scan_ref as R
from thrill_amd.pipeline import exchange_totals, scan_carry, scan_identity

WORLD = 3
# ragged shards, the middle rank empty
BOUNDS = [0, 1237, 1237, 3001]
INITIAL = {R.U64: 0x0123456789ABCDEF, R.I64: 0xFFFFFFFFFFFFFF85,   # -123
           R.F64: 0xC045000000000000}                              # -42.0
CASES = [(op, vt, ex) for op, vt in R.VALID for ex in (0, 1)]


def _data(vt):
    return R.values(BOUNDS[-1], vt, seed=0x5CA0 + vt)


def _worker(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        out = {}
        for op, vt, ex in CASES:
            shard = _data(vt)[BOUNDS[rank]:BOUNDS[rank + 1]]
            totals = exchange_totals(dist, R.fold(shard, op, vt), world)
            assert len(totals) == world
            assert totals[1] == R.identity(op, vt) == scan_identity(op, vt)
            carry = scan_carry(totals, rank, op, vt, INITIAL[vt])
            if rank == 0:
                assert carry == INITIAL[vt]
            out[(op, vt, ex)] = (R.scan(shard, op, vt, ex, carry).tobytes(),
                                 scan_carry(totals, world, op, vt,
                                            R.identity(op, vt)))
        q.put((rank, out))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # surface the failure to the parent
        q.put((rank, f"ERROR: {e!r}"))
        raise


def test_distributed_prefix_sum_protocol_world3():
    ctxm = mp.get_context("spawn")
    q = ctxm.Queue()
    procs = [ctxm.Process(target=_worker, args=(r, WORLD, 29741, q))
             for r in range(WORLD)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(WORLD):
        rank, out = q.get(timeout=180)
        assert not isinstance(out, str), out
        results[rank] = out
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for op, vt, ex in CASES:
        x = _data(vt)
        got = np.concatenate([
            np.frombuffer(results[r][(op, vt, ex)][0], np.uint64)
            for r in range(WORLD)])
        expect = R.scan(x, op, vt, ex, INITIAL[vt])
        assert np.array_equal(got, expect), (op, vt, ex)
        # the all-rank fold every rank derives from the same totals
        for r in range(WORLD):
            assert results[r][(op, vt, ex)][1] == R.fold(x, op, vt)


def test_scan_carry_is_pure_host_arithmetic():
    # rank 0 starts from the initial value whatever the totals are
    for op, vt in R.VALID:
        assert scan_carry([5, 6, 7], 0, op, vt, 99) == 99
    assert scan_carry([5, 6, 7], 2, R.SUM, R.U64, (1 << 64) - 1) == 10
    assert scan_carry([5, 6, 7], 3, R.MAX, R.U64, 0) == 7
    # signed and double orders, not the order of the raw bits
    neg5, neg1 = (1 << 64) - 5, 0xBFF0000000000000    # -5, -1.0
    assert scan_carry([3, neg5], 2, R.MIN, R.I64, 10) == neg5
    assert scan_carry([3, neg5], 2, R.MIN, R.U64, 10) == 3
    assert scan_carry([neg1, 0x4000000000000000], 2, R.MIN, R.F64,
                      0x3FF0000000000000) == neg1
    assert scan_carry([neg1], 1, R.MAX, R.F64, 0x8000000000000000) \
        == 0x8000000000000000                          # -0.0 > -1.0
