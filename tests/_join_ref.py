"""numpy restatement of the device inner join's semantics — the checker of
the join tests, independent of the code under test.

join(lkeys, rkeys) -> (li, ri): all index pairs (i, j) with lkeys[i] ==
rkeys[j], ordered by key ascending as unsigned 64-bit, then i ascending,
then j ascending (include/thrill_amd.h "InnerJoin"). Stable argsort of both
sides, searchsorted left and right, repeat.
"""
import numpy as np


def join(lkeys, rkeys):
    lk = np.asarray(lkeys, dtype=np.uint64)
    rk = np.asarray(rkeys, dtype=np.uint64)
    lo_ = np.argsort(lk, kind="stable")
    ro_ = np.argsort(rk, kind="stable")
    ls, rs = lk[lo_], rk[ro_]
    lo = np.searchsorted(rs, ls, side="left").astype(np.int64)
    hi = np.searchsorted(rs, ls, side="right").astype(np.int64)
    cnt = hi - lo
    total = int(cnt.sum())
    li = np.repeat(lo_, cnt)
    # row p of element e is right row lo[e] + (p - off[e])
    off = np.cumsum(cnt) - cnt
    within = np.arange(total, dtype=np.int64) - np.repeat(off, cnt)
    ri = ro_[np.repeat(lo, cnt) + within] if total else ro_[:0]
    return li.astype(np.uint32), ri.astype(np.uint32)


def total(lkeys, rkeys):
    """number of result pairs, without materialising them."""
    lk = np.sort(np.asarray(lkeys, dtype=np.uint64))
    rk = np.sort(np.asarray(rkeys, dtype=np.uint64))
    return int((np.searchsorted(rk, lk, side="right") -
                np.searchsorted(rk, lk, side="left")).sum())


def brute(lkeys, rkeys):
    """the definition, by a double loop: for the small cases that check
    join() itself."""
    lk = [int(k) for k in lkeys]
    rk = [int(k) for k in rkeys]
    rows = [(lk[i], i, j) for i in range(len(lk)) for j in range(len(rk))
            if lk[i] == rk[j]]
    rows.sort()
    return (np.array([r[1] for r in rows], dtype=np.uint32),
            np.array([r[2] for r in rows], dtype=np.uint32))
