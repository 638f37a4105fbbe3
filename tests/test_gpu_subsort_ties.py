"""GPU tests of the tie count inside the single-wave sub-bucket sort
(k_wave16_sort_sub, record form) of the two-level 9-bit MSB flow.

On the record path the sub-sort counts keys equal to their neighbour while
it holds a sub-bucket sorted, and writes sorted keys back only for
sub-buckets that hold a tie; t9_sort_last_tiecount says whether that count
(1) or the standalone pass over the sorted keys (0) decided if the tie
machinery runs. A missed tie is visible: the radix pipeline is stable, so
equal-prefix records come out in input order, and every input here gives
tied records tails that DESCEND in input order.

Inputs are built from a handful of top-17-bit prefixes (sub-bucket =
top 17 bits of the big-endian 8-byte prefix), the low 47 key bits encode the
intended sorted position inside the sub-bucket, and the record order is
shuffled with a seed. Every case checks on the host that the sub-bucket
sizes are the intended ones, so none silently takes another path."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tests import _gpu as G
    from thrill_amd import Native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSUB9 = 256 * 512

# filler sub-buckets (no ties) that lift every input above the 2^14 records
# at which T9_SORT_ALGO=msb takes the MSB path; strictly between the
# smallest and the largest prefix the cases plant
FILL = [(1000 + 7001 * i, 1000, []) for i in range(17)]
FIRST, MID, LAST = 0, 70001, NSUB9 - 1


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = Native(device=0)
    yield n
    n.close()


@pytest.fixture(autouse=True)
def msb_env():
    names = ("T9_SORT_ALGO", "T9_FUSED_EXTRACT", "T9_SORT_OVERLAP",
             "T9_PASS2_BITS", "T9_MSB_LEVELS", "T9_EXTRACT_HIST",
             "T9_LDS_WAVE16")
    saved = {k: os.environ.get(k) for k in names}
    for k in names:
        os.environ.pop(k, None)
    os.environ["T9_SORT_ALGO"] = "msb"
    yield
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def make_keys(subs):
    """subs: (prefix17, ns, runs); runs: (q, m) = sorted positions
    q..q+m-1 of the sub-bucket share one key; runs == "equal" = every key
    of the sub-bucket is the same. Returns keys in sorted order."""
    out = []
    for pre, ns, runs in subs:
        rank = np.arange(ns, dtype=np.uint64)
        if runs == "equal":
            rank[:] = 5
        else:
            for q, m in runs:
                assert q + m <= ns
                rank[q:q + m] = q
        out.append((np.uint64(pre) << np.uint64(47)) | rank)
    return np.concatenate(out)


def make_records(subs, seed, rs=100, le=False):
    keys = make_keys(subs)
    n = len(keys)
    rng = np.random.default_rng(seed)
    keys = keys[rng.permutation(n)]
    recs = rng.integers(0, 256, (n, rs)).astype(np.uint8)
    recs[:, :8] = keys.astype("<u8" if le else ">u8").view(np.uint8) \
        .reshape(n, 8)
    # tails descend in input order: equal-prefix records left in input
    # order (a missed tie) are in the wrong order
    tail = (np.uint64(1) << np.uint64(40)) - np.arange(n, dtype=np.uint64)
    recs[:, 8:16] = tail.astype(">u8").view(np.uint8).reshape(n, 8)
    return recs, keys


def check_sizes(keys, subs):
    """the sub-bucket sizes the device will see are the intended ones"""
    pre, cnt = np.unique(keys >> np.uint64(47), return_counts=True)
    want = {}
    for p, ns, _ in subs:
        want[p] = want.get(p, 0) + ns
    assert dict(zip(pre.tolist(), cnt.tolist())) == want
    assert len(keys) >= 1 << 14


def n_tied(keys):
    s = np.sort(keys)
    return int(np.count_nonzero(s[1:] == s[:-1]))


def gpu_sort(nat, recs, keyle=False):
    n, rs = recs.shape
    din = G.dev(recs.reshape(-1))
    dout = G.empty(n * rs, np.uint8)
    w = G.ws(nat.ws("sort_records", n, rs))
    if keyle:
        nat.sort_records_keyle(G.ptr(din), G.ptr(dout), n, rs, G.ptr(w),
                               G.stream())
    else:
        nat.sort_records(G.ptr(din), G.ptr(dout), n, rs, 10, G.ptr(w),
                         G.stream())
    return G.host(dout, np.uint8).reshape(n, rs), nat.sort_last_tiecount()


def run_case(nat, oracle, subs, seed, path, ties):
    recs, keys = make_records(subs, seed)
    check_sizes(keys, subs)
    assert n_tied(keys) == ties
    got, how = gpu_sort(nat, recs)
    assert how == path
    assert np.array_equal(got, oracle.sort_records(recs))


# name -> (sub-buckets, tied neighbour pairs); all on the in-kernel count
CASES = {
    # planted pair positions (q, q + 1)
    "inside_lane": (FILL + [(MID, 700, [(37, 2)])], 1),
    "straddles_lanes": (FILL + [(MID, 700, [(16 * 9 - 1, 2)])], 1),
    "last_pair_before_pads": (FILL + [(MID, 700, [(698, 2)])], 1),
    "ns2_is_one_tie": (FILL + [(MID, 2, [(0, 2)])], 1),
    "first_and_last_sub_bucket":
        (FILL + [(FIRST, 300, [(0, 2)]), (LAST, 300, [(298, 2)])], 2),
    "run_of_three": (FILL + [(MID, 700, [(100, 3)])], 2),
    "run_of_three_over_lanes": (FILL + [(MID, 700, [(15, 3)])], 2),
    # sizes, with and without a tie
    "ns1": (FILL + [(MID, 1, [])], 0),
    "ns2_no_tie": (FILL + [(MID, 2, [])], 0),
    "ns1023_no_tie": (FILL + [(MID, 1023, [])], 0),
    "ns1023_tie": (FILL + [(MID, 1023, [(1021, 2)])], 1),
    "ns1024_no_tie": (FILL + [(MID, 1024, [])], 0),
    "ns1024_tie_at_end": (FILL + [(MID, 1024, [(1022, 2)])], 1),
    "ns1024_tie_at_start": (FILL + [(MID, 1024, [(0, 2)])], 1),
    # every key of the sub-bucket equal: the early-return branch
    "all_equal_low48": (FILL + [(MID, 333, "equal")], 332),
    "all_equal_and_a_pair":
        (FILL + [(MID, 64, "equal"), (LAST, 500, [(255, 2)])], 64),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_counted_in_sub_sort(nat, oracle, name):
    subs, ties = CASES[name]
    run_case(nat, oracle, subs, 0x7100 + len(name), 1, ties)


def test_1025_takes_standalone_count(nat, oracle):
    # default limit of the single-wave sort is 1024: another sub-sort runs,
    # the standalone pass counts, and the tie is still found
    subs = FILL + [(MID, 1025, [(1023, 2)])]
    run_case(nat, oracle, subs, 0x7201, 0, 1)


def test_8bit_pass2_takes_standalone_count(nat, oracle):
    os.environ["T9_PASS2_BITS"] = "8"
    recs, keys = make_records(FILL + [(MID, 700, [(37, 2)])], 0x7203)
    got, how = gpu_sort(nat, recs)
    assert how == 0
    assert np.array_equal(got, oracle.sort_records(recs))


@pytest.mark.parametrize("n", [1 << 14, 100001])
def test_uniform_no_ties(nat, oracle, n):
    recs = oracle.gen_records(n, seed=0x0713 + n)
    keys = recs[:, :8].copy().view(">u8").reshape(-1).astype(np.uint64)
    assert n_tied(keys) == 0, "seed has equal prefixes"
    assert np.unique(keys >> np.uint64(47), return_counts=True)[1].max() \
        <= 1024
    got, how = gpu_sort(nat, recs)
    assert how == 1
    assert np.array_equal(got, oracle.sort_records(recs))


def test_overlapped_schedule_counts_in_sub_sort(nat, oracle):
    os.environ["T9_SORT_OVERLAP"] = "1"
    subs, ties = CASES["first_and_last_sub_bucket"]
    recs, keys = make_records(subs, 0x7204)
    got, how = gpu_sort(nat, recs)
    assert how == 1
    assert np.array_equal(got, oracle.sort_records(recs))
    recs = oracle.gen_records(100001, seed=0x0713 + 100001)
    got, how = gpu_sort(nat, recs)
    assert how == 1 and nat.sort_last_schedule() > 0
    assert np.array_equal(got, oracle.sort_records(recs))


def test_128_byte_records(nat, oracle):
    subs = FILL + [(MID, 700, [(16 * 9 - 1, 2)])]
    recs, keys = make_records(subs, 0x7205, rs=128)
    check_sizes(keys, subs)
    got, how = gpu_sort(nat, recs)
    assert how == 1
    assert np.array_equal(got, oracle.sort_records(recs))


def test_keyle_records(nat):
    subs = FILL + [(MID, 700, [(16 * 9 - 1, 2)])]
    recs, keys = make_records(subs, 0x7206, le=True)
    check_sizes(keys, subs)
    got, how = gpu_sort(nat, recs, keyle=True)
    assert how == 1
    order = np.lexsort(tuple(recs[:, c] for c in range(99, 7, -1))
                       + (keys,))
    assert np.array_equal(got, recs[order])


@pytest.mark.parametrize("name", ["straddles_lanes", "all_equal_low48",
                                  "ns1024_tie_at_end", "ns1"])
def test_pair_sort_keeps_sorted_keys(nat, name):
    # the public pair sort runs the same kernel without the record flags:
    # keys fully sorted, values stable
    keys = make_records(CASES[name][0], 0x7300 + len(name))[1]
    n = len(keys)
    vals = np.arange(n, dtype=np.uint32)
    dk, dv = G.dev(keys), G.dev(vals)
    w = G.ws(nat.ws("sort_pairs", n))
    nat.sort_pairs_u64_u32(G.ptr(dk), G.ptr(dv), n, G.ptr(w), G.stream())
    assert np.array_equal(G.host(dk, np.uint64), np.sort(keys))
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(G.host(dv, np.uint32), vals[order])


# ---- the 2048 and 4096 tiers (several waves per block) ----------------
# T9_WAVE16_MAX is latched at first use, so these run in ONE fresh child
# process that sets it to 4096.

TIER_CASES = {
    # largest sub-bucket 2048 -> the 2048 tier, waves of 1024 elements
    "tier2048": (FILL + [(FIRST, 1025, [(1023, 2)]),
                         (MID, 2048, [(2046, 2), (15, 2)]),
                         (LAST, 1500, [])], 3),
    "tier2048_no_tie": (FILL + [(MID, 2048, []), (LAST, 1025, [])], 0),
    # largest sub-bucket 4096 -> the 4096 tier
    "tier4096": (FILL + [(FIRST, 4095, [(4093, 2)]),
                         (MID, 4096, [(1023, 2), (4094, 2), (2047, 3)]),
                         (LAST, 1025, [(1023, 2)])], 6),
    "tier4096_no_tie": (FILL + [(MID, 4095, []), (LAST, 4096, [])], 0),
}


def _child_main():
    from tests._oracle import Oracle
    oracle = Oracle()
    nat = Native(device=0)
    os.environ["T9_SORT_ALGO"] = "msb"
    for name in sorted(TIER_CASES):
        subs, ties = TIER_CASES[name]
        run_case(nat, oracle, subs, 0x7400 + len(name), 1, ties)
        # the pair sort through the same tier keeps fully sorted keys
        keys = make_records(subs, 0x7500)[1]
        vals = np.arange(len(keys), dtype=np.uint32)
        dk, dv = G.dev(keys), G.dev(vals)
        w = G.ws(nat.ws("sort_pairs", len(keys)))
        nat.sort_pairs_u64_u32(G.ptr(dk), G.ptr(dv), len(keys), G.ptr(w),
                               G.stream())
        assert np.array_equal(G.host(dk, np.uint64), np.sort(keys)), name
        assert np.array_equal(G.host(dv, np.uint32),
                              vals[np.argsort(keys, kind="stable")]), name
        print("tier case ok:", name, flush=True)
    nat.close()
    print("TIERS-OK", flush=True)


def test_tiers_2048_and_4096():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = dict(os.environ)
    for k in ("T9_FUSED_EXTRACT", "T9_SORT_OVERLAP", "T9_PASS2_BITS",
              "T9_MSB_LEVELS", "T9_EXTRACT_HIST", "T9_LDS_WAVE16"):
        env.pop(k, None)
    env["T9_WAVE16_MAX"] = "4096"
    code = ("import sys; sys.path.insert(0, %r); "
            "from tests import test_gpu_subsort_ties as T; T._child_main()"
            % REPO)
    r = subprocess.run([sys.executable, "-s", "-c", code], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "TIERS-OK" in r.stdout, \
        r.stdout[-2000:] + r.stderr[-4000:]
