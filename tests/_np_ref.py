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
