#!/usr/bin/env python3
"""Reduce-operator build rate (secondary measurement, not the driver bench
line): one Zipf(1.1) token stream, 2^28 tokens over a 10M vocabulary,
value = token index, reduced into the u64 table by t9_reduce_build_op with
SUM, MIN and MAX — and, for reference, by the plain t9_reduce_build.

Each repeat times ONE build with device events (init_op runs before the
start event); the variants alternate inside every repeat, starting from a
different one each time, so that drift of a shared machine and the
predecessor kernel hit all of them alike. The claim under test: MIN and MAX
lie within the SUM runs' own spread (min..max over the repeats).

    python scripts/bench_reduce_ops.py [--log2n 28] [--repeats 7] [--out F]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from thrill_amd import Native, T9_OP_MAX, T9_OP_MIN, T9_OP_SUM, T9_VAL_U64  # noqa: E402
from thrill_amd.pipeline import zipf_cdf  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2n", type=int, default=28)
ap.add_argument("--vocab", type=int, default=10_000_000)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.repeats >= 5, "at least five repeats"
assert torch.cuda.is_available(), "needs a GPU (no CPU fallback)"

n, vocab = 1 << args.log2n, args.vocab
nat = Native(device=0)
ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
stream = lambda: ctypes.c_void_p(  # noqa: E731
    torch.cuda.current_stream().cuda_stream)

d_cdf = torch.from_numpy(zipf_cdf(vocab, 1.1)).cuda()
d_toks = torch.empty(n, dtype=torch.int64, device="cuda")
nat.zipf_tokens(ptr(d_toks), ptr(d_cdf), vocab, 0, n, 0x44, stream())
d_vals = torch.arange(n, dtype=torch.int64, device="cuda")
cap = 1 << (2 * vocab + 2 - 1).bit_length()
d_tbl = torch.empty(2 * (cap + 1), dtype=torch.int64, device="cuda")
d_ok = torch.empty(cap + 1, dtype=torch.int64, device="cuda")
d_ov = torch.empty(cap + 1, dtype=torch.int64, device="cuda")
d_err = torch.empty(1, dtype=torch.int32, device="cuda")
d_n = torch.empty(1, dtype=torch.int64, device="cuda")

VARIANTS = [("sum", T9_OP_SUM), ("min", T9_OP_MIN), ("max", T9_OP_MAX),
            ("legacy_sum", None)]


def build(op, timed):
    s = stream()
    if op is None:
        nat.reduce_init(ptr(d_tbl), cap, s)
    else:
        nat.reduce_init_op(ptr(d_tbl), cap, op, T9_VAL_U64, s)
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    if op is None:
        nat.reduce_build(ptr(d_toks), ptr(d_vals), n, ptr(d_tbl), cap, 0,
                         ptr(d_err), s)
    else:
        nat.reduce_build_op(ptr(d_toks), ptr(d_vals), n, ptr(d_tbl), cap, 0,
                            op, T9_VAL_U64, ptr(d_err), s)
    b.record()
    torch.cuda.synchronize()
    assert int(d_err.item()) == 0, "table overflow"
    return a.elapsed_time(b) if timed else None


def drained(op):
    s = stream()
    if op is None:
        nat.reduce_drain(ptr(d_tbl), cap, ptr(d_ok), ptr(d_ov), ptr(d_n), s)
    else:
        nat.reduce_drain_op(ptr(d_tbl), cap, op, T9_VAL_U64, ptr(d_ok),
                            ptr(d_ov), ptr(d_n), s)
    m = int(d_n.item())
    order = torch.argsort(d_ok[:m])
    return d_ok[:m][order], d_ov[:m][order]


# the variants must agree with each other before their times mean anything
uniques = None
checks = {}
for name, op in VARIANTS:
    for _ in range(args.warmup):
        build(op, False)
    k, v = drained(op)
    if uniques is None:
        uniques, keys0 = len(k), k
    assert len(k) == uniques and torch.equal(k, keys0), name
    checks[name] = v
assert torch.equal(checks["sum"], checks["legacy_sum"])
M64 = (1 << 64) - 1
assert int(checks["sum"].sum().item()) & M64 == (n * (n - 1) // 2) & M64
assert bool((checks["min"] <= checks["max"]).all())
# a word seen once has first == last occurrence == its value under SUM
once = checks["min"] == checks["max"]
assert torch.equal(checks["sum"][once], checks["min"][once])

times = {name: [] for name, _ in VARIANTS}
for r in range(args.repeats):
    # rotate the starting variant so that no variant always follows the
    # same predecessor
    k = r % len(VARIANTS)
    for name, op in VARIANTS[k:] + VARIANTS[:k]:
        times[name].append(round(build(op, True), 4))

res = {
    "metric": "t9_reduce_build_op ms per build (u64 table)",
    "device": torch.cuda.get_device_name(0),
    "tokens": n, "vocab": vocab, "zipf_s": 1.1, "uniques": uniques,
    "capacity": cap, "repeats": args.repeats,
    "timing": "device events around one build; variants alternate "
              "within each repeat, rotating the first",
}
for name, ts in times.items():
    st = sorted(ts)
    res[name] = {"ms": ts, "min": st[0], "median": st[len(st) // 2],
                 "max": st[-1],
                 "tokens_per_s_median": round(n / (st[len(st) // 2] * 1e-3))}
lo, hi = res["sum"]["min"], res["sum"]["max"]
res["within_sum_spread"] = {
    name: bool(lo <= res[name]["median"] <= hi) for name in ("min", "max")}
nat.close()
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
