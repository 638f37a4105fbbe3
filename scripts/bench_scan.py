#!/usr/bin/env python3
"""Scan-family rate (secondary measurement, not the driver bench line):
2^28 u64 on one GPU through t9_scan_u64 (inclusive SUM, inclusive MAX, and
SUM with pass 1 visiting the tiles in reverse — the A/B of
T9_SCAN_P1_REVERSE), t9_scan_kv MAX over 2^27 pairs (the same bytes) and
t9_fold_u64, next to two yardsticks that are not the code under test: a
device-to-device copy of the same bytes (tensor.copy_) and torch.cumsum on
the same int64 tensor.

Each repeat times ONE call per variant with device events; the variants
alternate inside every repeat, starting from a different one each time, so
that drift of a shared machine and the predecessor kernel hit all of them
alike. The share of the middle pass comes from the library's own perf
classes ("scan", "scan_pass2") in a separate, untimed set of calls.

    python scripts/bench_scan.py [--log2n 28] [--repeats 7] [--out F]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from thrill_amd import Native, T9_OP_MAX, T9_OP_SUM, T9_VAL_U64  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2n", type=int, default=28)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.repeats >= 5, "at least five repeats"
assert torch.cuda.is_available(), "needs a GPU (no CPU fallback)"

n = 1 << args.log2n
nat = Native(device=0)
ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
stream = lambda: ctypes.c_void_p(  # noqa: E731
    torch.cuda.current_stream().cuda_stream)

d_in = torch.empty(n, dtype=torch.int64, device="cuda")
nat.gen_u64(ptr(d_in), 0, n, 0x5CA9, stream())
d_out = torch.empty(n, dtype=torch.int64, device="cuda")
d_ws = torch.empty(int(nat.ws("scan", n)), dtype=torch.uint8, device="cuda")
d_res = torch.empty(1, dtype=torch.int64, device="cuda")


def scan(op, reverse=False):
    if reverse:
        os.environ["T9_SCAN_P1_REVERSE"] = "1"
    nat.scan_u64(ptr(d_in), ptr(d_out), n, op, T9_VAL_U64, 0, 0, None,
                 ptr(d_ws), stream())
    os.environ.pop("T9_SCAN_P1_REVERSE", None)


VARIANTS = [
    ("scan_sum", lambda: scan(T9_OP_SUM)),
    ("scan_max", lambda: scan(T9_OP_MAX)),
    ("scan_sum_p1_reverse", lambda: scan(T9_OP_SUM, reverse=True)),
    ("scan_kv_max", lambda: nat.scan_kv(
        ptr(d_in), ptr(d_out), n // 2, T9_OP_MAX, T9_VAL_U64, 0, None,
        ptr(d_ws), stream())),
    ("fold_sum", lambda: nat.fold_u64(
        ptr(d_in), n, 1, T9_OP_SUM, T9_VAL_U64, ptr(d_res), ptr(d_ws),
        stream())),
    ("copy", lambda: d_out.copy_(d_in)),
    ("torch_cumsum", lambda: torch.cumsum(d_in, 0, out=d_out)),
]


def timed(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


# the scan must agree with the yardstick before its time means anything
torch.cumsum(d_in, 0, out=d_out)
expect_tail = d_out[-4096:].clone()
expect_mid = d_out[n // 2 - 1:n // 2 + 4097].clone()
for rev in (False, True):
    scan(T9_OP_SUM, reverse=rev)
    assert torch.equal(d_out[-4096:], expect_tail), "scan != torch.cumsum"
    assert torch.equal(d_out[n // 2 - 1:n // 2 + 4097], expect_mid)
nat.fold_u64(ptr(d_in), n, 1, T9_OP_SUM, T9_VAL_U64, ptr(d_res), ptr(d_ws),
             stream())
assert int(d_res.item()) == int(expect_tail[-1].item()), "fold != cumsum[-1]"

for _, fn in VARIANTS:
    for _ in range(args.warmup):
        fn()
torch.cuda.synchronize()

times = {name: [] for name, _ in VARIANTS}
for r in range(args.repeats):
    k = r % len(VARIANTS)
    for name, fn in VARIANTS[k:] + VARIANTS[:k]:
        times[name].append(round(timed(fn), 4))

# share of the middle pass, from the library's perf classes
nat.perf_reset()
nat.perf_enable(True)
for _ in range(5):
    scan(T9_OP_SUM)
torch.cuda.synchronize()
all_ms, calls = nat.perf_read("scan")
p2_ms, _ = nat.perf_read("scan_pass2")
nat.perf_enable(False)
nat.perf_reset()

res = {
    "metric": "scan family, ms per call",
    "device": torch.cuda.get_device_name(0),
    "elements": n, "bytes": 8 * n, "repeats": args.repeats,
    "geometry": dict(zip(("tile_elems", "partials_per_block"),
                         nat.scan_geometry())),
    "timing": "device events around one call; variants alternate within "
              "each repeat, rotating the first",
}
for name, ts in times.items():
    st = sorted(ts)
    med = st[len(st) // 2]
    res[name] = {"ms": ts, "min": st[0], "median": med, "max": st[-1],
                 "GB_per_s_of_input_median": round(8 * n / (med * 1e-3) / 1e9,
                                                   1)}
res["pass2_share_of_scan"] = round(p2_ms / all_ms, 4) if all_ms else None
res["pass2_ms_per_call"] = round(p2_ms / max(calls, 1), 4)
res["scan_ms_per_call_perf_class"] = round(all_ms / max(calls, 1), 4)
res["ratio_scan_sum_to_copy"] = round(
    res["scan_sum"]["median"] / res["copy"]["median"], 3)
res["ratio_scan_sum_to_torch_cumsum"] = round(
    res["scan_sum"]["median"] / res["torch_cumsum"]["median"], 3)
res["predicted_ratio_scan_to_copy_from_traffic"] = 1.5
lo, hi = res["scan_sum"]["min"], res["scan_sum"]["max"]
res["p1_reverse_median_within_forward_spread"] = bool(
    lo <= res["scan_sum_p1_reverse"]["median"] <= hi)
nat.close()
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
