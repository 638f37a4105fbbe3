#!/usr/bin/env python3
"""Inner-join stage times (secondary measurement, not the driver bench
line): 2^26 x 2^26 unique shuffled u64 keys on one GPU, so 2^26 result rows.

  (a) sorts      the two (key, iota) pair sorts alone — existing kernels,
                 the yardstick, timed in the same session
  (b) bounds     k_join_bounds            (perf class "join_bounds")
  (c) scan       t9_scan_u64 over cnt     (perf class "scan")
  (d) emit       k_join_emit              (device events around the call)

and the emit alone on three skewed inputs of the same output size: one hot
key 2^13 x 2^13, 2^26 x 1 on one key, and 1 x 2^26 on one key (one left
element spread over every output tile).

Each repeat times ONE call per variant with device events; the variants
alternate inside every repeat, starting from a different one each time.
Two A/B pairs ride along: k_join_bounds with the plain binary search for
the upper bound (T9_JOIN_GALLOP=0) and k_join_emit writing one position per
lane instead of four (T9_JOIN_EMIT_V4=0).
(b) and (c) come from the library's perf classes, recorded inside the
count call of the same repeat. Model bytes: bounds 8 B per left key + 8 B
per right key + 12 B written per left element; scan 24 B per element;
emit 12 + 4 + 4 B read and 8 B written per row.

    python scripts/bench_join.py [--log2n 26] [--repeats 7] [--out F]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from thrill_amd import Native  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2n", type=int, default=26)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.repeats >= 7, "at least seven repeats"
assert args.log2n % 2 == 0, "the hot-key input is 2^(log2n/2) squared"
assert torch.cuda.is_available(), "needs a GPU (no CPU fallback)"

n = 1 << args.log2n
h = 1 << (args.log2n // 2)
nat = Native(device=0)
ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
stream = lambda: ctypes.c_void_p(  # noqa: E731
    torch.cuda.current_stream().cuda_stream)
i64, i32 = torch.int64, torch.int32
GOLD = -7046029254386353131   # 0x9E3779B97F4A7C15: odd, so k -> k * GOLD
                              # is a bijection of the 64-bit words


def unique_keys(seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randperm(n, generator=g, device="cuda", dtype=i64) * GOLD


class Case:
    """one input with its join state: count() redoes t9_join_count,
    emit() runs t9_join_emit on the state of the last count."""

    def __init__(self, lk, rk):
        self.lk, self.rk = lk, rk
        self.nl, self.nr = lk.numel(), rk.numel()
        self.ws = torch.empty(int(nat.ws("join", self.nl, self.nr)),
                              dtype=torch.uint8, device="cuda")
        self.total = self.count()

    def count(self):
        return nat.join_count(ptr(self.lk), self.nl, ptr(self.rk), self.nr,
                              ptr(self.ws), stream())

    def emit(self):
        nat.join_emit(self.nl, self.nr, ptr(self.ws), self.total,
                      ptr(out_l), ptr(out_r), stream())


out_l = torch.empty(n, dtype=i32, device="cuda")
out_r = torch.empty(n, dtype=i32, device="cuda")
hot = torch.full((h,), 12345, dtype=i64, device="cuda")
one = torch.full((1,), 12345, dtype=i64, device="cuda")
many = torch.full((n,), 12345, dtype=i64, device="cuda")
uniq = Case(unique_keys(1), unique_keys(2))
hot_case = Case(hot, hot)
left_many = Case(many, one)
right_many = Case(one, many)
pos = torch.arange(n, device="cuda", dtype=i64)

# the results must be right before their times mean anything
assert uniq.total == n
uniq.emit()
kl, kr = uniq.lk[out_l.long()], uniq.rk[out_r.long()]
assert torch.equal(kl, kr), "unique: joined keys differ"
u = kl ^ (-1 << 63)   # unsigned order as signed
assert bool((u[1:] > u[:-1]).all()), "unique: keys not ascending"
del kl, kr, u
assert hot_case.total == n
hot_case.emit()
assert torch.equal(out_l.long(), pos // h) and \
    torch.equal(out_r.long(), pos % h), "hot key: wrong rows"
assert left_many.total == n
left_many.emit()
assert torch.equal(out_l.long(), pos) and int(out_r.max()) == 0
assert right_many.total == n
right_many.emit()
assert torch.equal(out_r.long(), pos) and int(out_l.max()) == 0
del pos

# (a): what t9_join_count does before its own kernels, on scratch buffers
s_k = torch.empty(n, dtype=i64, device="cuda")
s_i = torch.empty(n, dtype=i32, device="cuda")
s_ws = torch.empty(int(nat.ws("sort_pairs", n)), dtype=torch.uint8,
                   device="cuda")


def sorts():
    for keys in (uniq.lk, uniq.rk):
        nat.extract_key64_le(ptr(keys), n, 8, 0, ptr(s_k), ptr(s_i),
                             stream())
        nat.sort_pairs_u64_u32(ptr(s_k), ptr(s_i), n, ptr(s_ws), stream())


perf = {"bounds": [], "scan": [], "bounds_plain_search": []}


def count_unique(gallop=True):
    if not gallop:
        os.environ["T9_JOIN_GALLOP"] = "0"
    nat.perf_reset()
    nat.perf_enable(True)
    uniq.count()
    b_ms, b_n = nat.perf_read("join_bounds")
    s_ms, s_n = nat.perf_read("scan")
    nat.perf_enable(False)
    nat.perf_reset()
    os.environ.pop("T9_JOIN_GALLOP", None)
    assert b_n == 1 and s_n == 1
    if gallop:
        perf["bounds"].append(round(b_ms, 4))
        perf["scan"].append(round(s_ms, 4))
    else:
        perf["bounds_plain_search"].append(round(b_ms, 4))


def scalar(case):
    """the emit writing one position per lane (T9_JOIN_EMIT_V4=0)."""
    def run():
        os.environ["T9_JOIN_EMIT_V4"] = "0"
        case.emit()
        os.environ.pop("T9_JOIN_EMIT_V4", None)
    return run


VARIANTS = [
    ("sorts", sorts),
    ("count_unique", count_unique),
    ("count_unique_plain_search", lambda: count_unique(gallop=False)),
    ("emit_unique", uniq.emit),
    ("emit_unique_1_per_lane", scalar(uniq)),
    ("emit_hot_key", hot_case.emit),
    ("emit_hot_key_1_per_lane", scalar(hot_case)),
    ("emit_left_many", left_many.emit),
    ("emit_right_many", right_many.emit),
]


def timed(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


for _, fn in VARIANTS:
    for _ in range(args.warmup):
        fn()
torch.cuda.synchronize()
perf = {k: [] for k in perf}

times = {name: [] for name, _ in VARIANTS}
for r in range(args.repeats):
    k = r % len(VARIANTS)
    for name, fn in VARIANTS[k:] + VARIANTS[:k]:
        times[name].append(round(timed(fn), 4))
times.update(perf)

MODEL = {   # bytes the algorithm needs per call
    "bounds": 8 * n + 8 * n + 12 * n,
    "bounds_plain_search": 8 * n + 8 * n + 12 * n,
    "emit_unique_1_per_lane": 28 * n, "emit_hot_key_1_per_lane": 28 * n,
    "scan": 24 * n,
    "emit_unique": 28 * n, "emit_hot_key": 28 * n,
    "emit_left_many": 28 * n, "emit_right_many": 28 * n,
}

res = {
    "metric": "inner join stages, ms per call",
    "device": torch.cuda.get_device_name(0),
    "n_left": n, "n_right": n, "rows": n, "repeats": args.repeats,
    "geometry": dict(zip(("left_tile", "out_tile", "stage_keys"),
                         nat.join_geometry())),
    "timing": "device events around one call; variants alternate within "
              "each repeat, rotating the first; bounds and scan from the "
              "perf classes inside count_unique",
}
for name, ts in times.items():
    st = sorted(ts)
    med = st[len(st) // 2]
    res[name] = {"ms": ts, "min": st[0], "median": med, "max": st[-1]}
    if name in MODEL:
        res[name]["model_bytes"] = MODEL[name]
        res[name]["model_GB_per_s_median"] = round(
            MODEL[name] / (med * 1e-3) / 1e9, 1)
res["sorts"]["Gkeys_per_s_median"] = round(
    2 * n / (res["sorts"]["median"] * 1e-3) / 1e9, 2)
own = sum(res[k]["median"] for k in ("bounds", "scan", "emit_unique"))
res["join_kernels_over_sorts"] = round(own / res["sorts"]["median"], 3)
base = res["emit_unique"]
for k in ("emit_hot_key", "emit_left_many", "emit_right_many"):
    res[k]["ns_per_row_median"] = round(res[k]["median"] * 1e6 / n, 4)
    res[k]["median_within_unique_spread"] = bool(
        base["min"] <= res[k]["median"] <= base["max"])
    res[k]["ratio_to_unique_median"] = round(
        res[k]["median"] / base["median"], 3)
base["ns_per_row_median"] = round(base["median"] * 1e6 / n, 4)
nat.close()
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
