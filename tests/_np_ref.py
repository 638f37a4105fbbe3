"""Vectorised numpy references of the sort and reduce support kernels, and
the kernel geometry the boundary-shape GPU tests are laid out around.

Every function restates one operation of include/thrill_amd.h in plain
numpy over uint64 / uint8 arrays; arithmetic wraps modulo 2^64 as it does
on the device. tests/test_np_ref_cpu.py pins these functions to the CPU
oracle and the constants below to the kernel sources."""
import numpy as np

# Geometry of the kernels under test (elements per block, grid caps). The
# GPU size ladders are built from these; test_np_ref_cpu.py reads the same
# numbers out of thrill_amd/csrc and fails if a kernel is retuned.
GRP_TILE = 8192          # t9_group.hip, keys per block
GRP_SCAN = 256           # block sums per trip of k_grp_scan
MRG_TILE = 4096          # t9_merge.hip, u64 outputs per block
MRG_SPAN = 16            # outputs per thread
MRG_REC_TILE = 1024      # records per block
MRG_REC_SPAN = 4         # records per thread
PAIRS_TILE = 2048        # t9_partition_idx, items per hist row
SCAN_CHUNK = 32          # hist rows per scan block
CHUNKSCAN_UNROLL = 16    # chunks per unrolled trip of k_chunkscan
CLASSIFY_GRID_CAP = 2048  # blocks of 256: second trip above 524 288 items
GRID_FOR_CAP = 4096      # t9_reduce.hip grid_for: second trip above 2^20
RECORDS_GRID_CAP = 16384  # extract / gather block cap
RED_LDS_PROBES = 4       # probes of a reduce build's per-block LDS filter
RED_LDS_DEFAULT = 4096   # LDS filter slots when no knob is set
RED_BUILD_GRID_CAP = 1024  # blocks of 256 of the LDS builds: second trip
#                            above 262 144 pairs

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
_K = np.uint64(0x9DDFEA08EB382D69)
_S47 = np.uint64(47)


def u64(x):
    return np.ascontiguousarray(x, dtype=np.uint64)


def hash128to64(upper, lower):
    """CityHash Hash128to64 (t9_common.h t9_hash128to64), elementwise."""
    upper, lower = u64(upper), u64(lower)
    with np.errstate(over="ignore"):
        a = (lower ^ upper) * _K
        a = a ^ (a >> _S47)
        b = (upper ^ a) * _K
        b = b ^ (b >> _S47)
        return b * _K


def hash2_of(ids):
    """t9_hash2_of: two hashes per id, the reserved all-ones remapped."""
    ids = u64(ids)
    out = []
    for base in (0x9AE16A3B2F90404F, 0xC3A5C85C97CB3127):
        h = hash128to64(np.full(ids.shape, base, np.uint64), ids)
        out.append(np.where(h == M64, h ^ np.uint64(1), h))
    return out[0], out[1]


def hash_bucket(keys, salt, p):
    keys = u64(keys)
    h = hash128to64(np.full(keys.shape, salt, np.uint64), keys)
    return (h % np.uint64(p)).astype(np.uint32)


def bucket_mod(keys, p):
    return (u64(keys) % np.uint64(p)).astype(np.uint32)


def _gidx(gidx0, n):
    with np.errstate(over="ignore"):
        return np.uint64(gidx0) + np.arange(n, dtype=np.uint64)


def classify(keys, gidx0, spl_k, spl_i):
    """bucket[i] = #{ j : (spl_k[j], spl_i[j]) < (keys[i], gidx0 + i) },
    pairs ordered lexicographically."""
    keys, spl_k, spl_i = u64(keys), u64(spl_k), u64(spl_i)
    g = _gidx(gidx0, len(keys))
    b = np.zeros(len(keys), np.uint32)
    for sk, si in zip(spl_k, spl_i):
        b += (sk < keys) | ((sk == keys) & (si < g))
    return b


def classify_rec(recs, gidx0, spl_recs, spl_i):
    """the same over whole records: byte-lexicographic record order, then
    the index. recs (n, rec_size) and spl_recs (p-1, rec_size) uint8."""
    recs = np.ascontiguousarray(recs, dtype=np.uint8)
    spl_recs = np.ascontiguousarray(spl_recs, dtype=np.uint8)
    spl_i = u64(spl_i)
    n = len(recs)
    g = _gidx(gidx0, n)
    rows = np.arange(n)
    b = np.zeros(n, np.uint32)
    for s, si in zip(spl_recs, spl_i):
        ne = recs != s
        first = ne.argmax(axis=1)           # 0 where the record equals s
        differs = ne[rows, first]
        less = np.where(differs, s[first] < recs[rows, first], si < g)
        b += less
    return b


def group_index(keys):
    """(unique keys, run start offsets) of a key-sorted array."""
    keys = u64(keys)
    if len(keys) == 0:
        return keys, np.empty(0, np.uint64)
    start = np.concatenate([[True], keys[1:] != keys[:-1]])
    off = np.flatnonzero(start).astype(np.uint64)
    return keys[start], off


def partition(bucket, p):
    """(stable permutation grouping items by bucket, p+1 start offsets)."""
    bucket = np.ascontiguousarray(bucket, dtype=np.uint32)
    perm = np.argsort(bucket, kind="stable").astype(np.uint32)
    cnt = np.bincount(bucket, minlength=p)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    return perm, off


def index_bucket(keys, begin, size, p):
    """bucket = (key - begin) * p / size; keys outside [begin, begin+size)
    go to the last cell's bucket and raise the flag. size * p < 2^64."""
    keys = u64(keys)
    with np.errstate(over="ignore"):
        g = keys - np.uint64(begin)
    bad = g >= np.uint64(size)
    g = np.where(bad, np.uint64(size - 1), g)
    b = (g * np.uint64(p) // np.uint64(size)).astype(np.uint32)
    return b, int(bad.any())


def reduce_by_index(keys, vals, begin, size):
    """dense[k - begin] += v (wrapping) over the keys in range; the flag is
    set if any key is outside [begin, begin+size)."""
    keys, vals = u64(keys), u64(vals)
    with np.errstate(over="ignore"):
        g = keys - np.uint64(begin)
        ok = g < np.uint64(size)
        dense = np.zeros(size, np.uint64)
        np.add.at(dense, g[ok].astype(np.int64), vals[ok])
    return dense, int(not ok.all())


def merge(a, b):
    return np.sort(np.concatenate([u64(a), u64(b)]), kind="stable")


def merge_records(A, B):
    """byte-lexicographic merge of two (n, rec_size) uint8 arrays, records
    of A before equal records of B."""
    cat = np.concatenate([A, B]).astype(np.uint8)
    src = np.concatenate([np.zeros(len(A), np.uint8),
                          np.ones(len(B), np.uint8)])
    # lexsort: the LAST key is the primary one
    keys = (src,) + tuple(cat[:, j] for j in range(cat.shape[1] - 1, -1, -1))
    return cat[np.lexsort(keys)]


def sort_records(recs):
    """records in byte-lexicographic order (to prepare merge inputs)."""
    recs = np.ascontiguousarray(recs, dtype=np.uint8)
    keys = tuple(recs[:, j] for j in range(recs.shape[1] - 1, -1, -1))
    return recs[np.lexsort(keys)]


# ------------------------------------------------- the reduce hash tables

_GOLD = np.uint64(0x9E3779B97F4A7C15)


def _salted(salt, keys):
    keys = u64(keys)
    return hash128to64(np.full(keys.shape, salt, np.uint64), keys)


def reduce_sum(keys, vals):
    """t9_reduce_* as a set: (sorted unique keys, wrapping u64 sums)."""
    keys, vals = u64(keys), u64(vals)
    if len(keys) == 0:
        return np.empty(0, np.uint64), np.empty(0, np.uint64)
    order = np.argsort(keys, kind="stable")
    uk, starts = np.unique(keys[order], return_index=True)
    return uk, np.add.reduceat(vals[order], starts)


def reduce128_sum(k1, k2, vals=None):
    """t9_reduce128_* as a set: (k1, k2, wrapping sum) triples in
    lexicographic (k1, k2) order; vals None counts 1 per pair."""
    k1, k2 = u64(k1), u64(k2)
    vals = np.ones(len(k1), np.uint64) if vals is None else u64(vals)
    if len(k1) == 0:
        return (np.empty(0, np.uint64),) * 3
    order = np.lexsort((k2, k1))
    s1, s2 = k1[order], k2[order]
    first = np.concatenate([[True], (s1[1:] != s1[:-1]) |
                            (s2[1:] != s2[:-1])])
    starts = np.flatnonzero(first)
    return s1[starts], s2[starts], np.add.reduceat(vals[order], starts)


def home_slot(keys, salt, cap):
    """where a key's probe chain starts in a global table of cap slots."""
    return _salted(salt, keys) & np.uint64(cap - 1)


def lds_slot(keys, salt, slots):
    """where it starts in a build's per-block LDS filter."""
    return (_salted(salt, keys) >> np.uint64(48)) & np.uint64(slots - 1)


def colliding_keys(salt, slots, lds_at, cap, home_at, count):
    """the first `count` keys i * 0x9E37..15, i in 1..2^22, whose LDS slot
    is lds_at (of `slots`) and whose home slot is home_at (of `cap`)."""
    with np.errstate(over="ignore"):
        cand = np.arange(1, (1 << 22) + 1, dtype=np.uint64) * _GOLD
    h = _salted(salt, cand)
    hit = (((h >> np.uint64(48)) & np.uint64(slots - 1)) ==
           np.uint64(lds_at)) & ((h & np.uint64(cap - 1)) ==
                                 np.uint64(home_at)) & (cand != M64)
    found = cand[hit]
    assert len(found) >= count, (len(found), count)
    return found[:count]


def _chains_unbroken(home, occupied):
    """every occupied slot is reached from its key's home slot without
    meeting an empty one (the walk wraps cap-1 -> 0)."""
    cap = len(occupied)
    at = np.flatnonzero(occupied)
    h = home[at].astype(np.int64)
    dist = (at - h) & (cap - 1)
    cum = np.concatenate([[0], np.cumsum(np.tile(~occupied, 2))])
    return np.all(cum[h + dist + 1] - cum[h] == 0)


def check_table_u64(raw, cap, salt):
    """a u64 table (2*(cap+1) words) read back from the device: every key
    sits in exactly one slot, and its probe chain from the home slot is
    unbroken. Returns the content as (sorted keys, their value words); the
    aux slot is not part of it."""
    raw = u64(raw)
    assert len(raw) == 2 * (cap + 1)
    keys, vals = raw[0:2 * cap:2], raw[1:2 * cap:2]
    occ = keys != M64
    k = keys[occ]
    assert len(np.unique(k)) == len(k), "a key occupies two slots"
    assert _chains_unbroken(home_slot(keys, salt, cap), occ), \
        "an empty slot between a key's home slot and its slot"
    order = np.argsort(k)
    return k[order], vals[occ][order]


def check_table_128(raw, cap, salt, stride=3):
    """the same for a 128-bit table of `stride` words per slot; no slot
    may hold a k1 without a k2. Returns (k1, k2, value words) in
    lexicographic order."""
    t = u64(raw)
    assert len(t) == stride * cap
    t = t.reshape(cap, stride)
    k1, k2, v = t[:, 0], t[:, 1], t[:, 2]
    occ = k1 != M64
    assert not np.any(occ & (k2 == M64)), "k1 claimed, k2 left empty"
    assert not np.any(~occ & (k2 != M64)), "k2 without a k1"
    pairs = np.stack([k1[occ], k2[occ]], axis=1)
    assert len(np.unique(pairs, axis=0)) == len(pairs), \
        "a composite key occupies two slots"
    assert _chains_unbroken(home_slot(k1, salt, cap), occ), \
        "an empty slot between a key's home slot and its slot"
    order = np.lexsort((k2[occ], k1[occ]))
    return k1[occ][order], k2[occ][order], v[occ][order]
