"""numpy restatement of the scan family's semantics — the checker of the
scan tests, independent of the code under test. Values travel as uint64
bit patterns; MIN and MAX run on the order-preserving encoding of
include/thrill_amd.h ("Reduce operators"), SUM on the raw bits (wrapping).
"""
import numpy as np

SUM, MIN, MAX = 0, 1, 2
U64, I64, F64 = 0, 1, 2
# every (op, vtype) the library accepts: SUM over F64 is refused
VALID = [(op, vt) for op in (SUM, MIN, MAX) for vt in (U64, I64, F64)
         if not (op == SUM and vt == F64)]
MSB = np.uint64(1 << 63)
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def enc(x, op, vt):
    x = np.asarray(x, dtype=np.uint64)
    if op == SUM or vt == U64:
        return x.copy()
    if vt == I64:
        return x ^ MSB
    return x ^ np.where(x >> np.uint64(63), ONES, MSB)


def dec(e, op, vt):
    e = np.asarray(e, dtype=np.uint64)
    if op == SUM or vt == U64:
        return e.copy()
    if vt == I64:
        return e ^ MSB
    return e ^ np.where(e >> np.uint64(63), MSB, ONES)


def identity(op, vt):
    """the fold of nothing, as a value of vt."""
    e = ONES if op == MIN else np.uint64(0)
    return int(dec(np.array([e], np.uint64), op, vt)[0])


def _acc(e, op):
    if op == SUM:
        return np.cumsum(e, dtype=np.uint64)
    if op == MIN:
        return np.minimum.accumulate(e)
    return np.maximum.accumulate(e)


def scan(x, op, vt, exclusive, initial):
    """out[i] = initial ⊕ x[0] ⊕ … ⊕ x[i] (exclusive: … ⊕ x[i-1])."""
    x = np.asarray(x, dtype=np.uint64)
    e = np.concatenate([enc(np.array([initial], np.uint64), op, vt),
                        enc(x, op, vt)])
    with np.errstate(over="ignore"):
        a = _acc(e, op)
    return dec(a[:-1] if exclusive else a[1:], op, vt)


def fold(x, op, vt):
    """x[0] ⊕ … ⊕ x[n-1]; the identity for n == 0."""
    x = np.asarray(x, dtype=np.uint64)
    if len(x) == 0:
        return identity(op, vt)
    with np.errstate(over="ignore"):
        return int(dec(_acc(enc(x, op, vt), op)[-1:], op, vt)[0])


def values(n, vt, seed):
    """n full-range patterns; I64 gets mixed signs by construction, F64
    gets ±0.0, ±inf, denormals and NaNs of both signs with payloads mixed
    in."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    if vt == F64 and n:
        special = np.array([
            0x0000000000000000, 0x8000000000000000,   # +0.0, -0.0
            0x7FF0000000000000, 0xFFF0000000000000,   # +inf, -inf
            0x0000000000000001, 0x800FFFFFFFFFFFFF,   # denormals
            0x7FF8000000000001, 0xFFF8000000000BAD,   # quiet NaNs
            0x7FF0000000000123, 0xFFF0000000000321,   # signalling NaNs
        ], dtype=np.uint64)
        where = rng.integers(0, n, size=min(n, max(1, n // 5)))
        x[where] = special[rng.integers(0, len(special), size=len(where))]
    return x
