#!/usr/bin/env python3
"""Cost of one short tie at bench scale for the fused sort + gather
(k_wave16_sort_gather): time t9_sort_records on 10 GiB of
  (a) uniform records (the bench input),
  (b) the same records with ONE duplicated 8-byte prefix, tails against the
      input order, planted in the last non-empty sub-bucket.
A library that settles short tie runs in the block keeps (b) at (a)
(fused = 1); one that does not pays the speculative fused gather and then
the tie path and a full gather (fused = 2). T9_SORT_FUSED_GATHER=0 gives
the separate-kernel reference. Prints one JSON line, seconds per case."""
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import _gpu as G           # noqa: E402
from thrill_amd import Native         # noqa: E402

REC = 100
N = int(os.environ.get("T9_TIES_N", 10 * 1024**3 // REC))


def time_sort(nat, din, dout, w, reps=5):
    s = G.stream()
    nat.sort_records(G.ptr(din), G.ptr(dout), N, REC, 10, G.ptr(w), s)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        nat.sort_records(G.ptr(din), G.ptr(dout), N, REC, 10, G.ptr(w), s)
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) / reps, 5), nat.sort_last_fused()


def main():
    nat = Native(device=0)
    din = G.empty(N * REC, np.uint8)
    dout = G.empty(N * REC, np.uint8)
    w = G.ws(nat.ws("sort_records", N, REC))
    out = {"records": N,
           "T9_SORT_FUSED_GATHER": os.environ.get("T9_SORT_FUSED_GATHER")}
    nat.gen_records(G.ptr(din), 0, N, 0x7421, G.stream())
    out["uniform_s"], out["uniform_fused"] = time_sort(nat, din, dout, w)

    # the record with the largest prefix lies in the last non-empty
    # sub-bucket; record `other` takes its prefix
    dk = G.empty(N, np.uint64)
    di = G.empty(N, np.uint32)
    nat.extract_key64(G.ptr(din), N, REC, 0, G.ptr(dk), G.ptr(di),
                      G.stream())
    home = int(torch.argmax(dk ^ (-2 ** 63)).item())
    del dk, di
    other = 12345 if home != 12345 else 12346
    v = din.view(N, REC)
    v[other, :8] = v[home, :8]
    lo, hi = min(home, other), max(home, other)
    v[lo, 8] = 0xFF
    v[hi, 8] = 0x00
    torch.cuda.synchronize()
    out["planted_s"], out["planted_fused"] = time_sort(nat, din, dout, w)
    out["planted_extra_ms"] = round(
        (out["planted_s"] - out["uniform_s"]) * 1e3, 3)
    # the planted pair is at the very end of the output, in tail order
    tail = dout.view(N, REC)[-3:].cpu().numpy()
    rows = [tuple(r) for r in tail]
    assert rows == sorted(rows), "planted tie not ordered"
    assert tail[-2, 8] == 0x00 and tail[-1, 8] == 0xFF
    print(json.dumps(out), flush=True)
    nat.close()


if __name__ == "__main__":
    main()
