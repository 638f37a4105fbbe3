/* t9_reduce_op.hip — the reduce tables with a selectable reduce operator
 * (SUM / MIN / MAX) over u64, i64 and f64 values, gfx950.
 *
 * The reference's reduce_function is any associative (V, V) -> V applied
 * in place (core/reduce_probing_hash_table.hpp:233); its own examples
 * reduce by key with std::max (examples/suffix_sorting/prefix_doubling.cpp).
 * Here the three operators that have a native 64-bit atomic run on the
 * device: atomicAdd / atomicMin / atomicMax on unsigned long long compile
 * to ds_{add,min,max}_u64 in LDS and global_atomic_{add,umin,umax}_x2 in
 * global memory — no compare-and-swap loop, so a MIN or MAX insert costs
 * the same atomic round trips as a SUM insert.
 *
 * Signed and double values ride the same two unsigned instructions
 * through an order-preserving encoding applied at load and undone at
 * drain:
 *   I64: bits ^ 0x8000000000000000            (two's-complement order)
 *   F64: bits ^ (sign ? ~0 : 0x8000000000000000)   (IEEE-754 totalOrder:
 *        -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN)
 * Both orders are total, so the result is bit-exact however the atomics
 * interleave. SUM is the wrapping add on the raw bits (identical for U64
 * and I64); SUM over F64 is refused — a floating atomic sum depends on
 * arrival order.
 *
 * Table layouts, capacity rules, the sentinel-key aux slot, probe order,
 * salt and the error model are those of t9_reduce.hip; only the value
 * word differs (identity-initialised, encoded for MIN/MAX). The legacy
 * SUM/U64 kernels stay in t9_reduce.hip untouched.
 */

#include "t9_common.h"
#include "thrill_amd.h"

#include <cstdlib>

#define T9_EMPTY 0xFFFFFFFFFFFFFFFFull

namespace {

/* t9_enc / t9_dec, the order-preserving value encoding, live in
 * t9_common.h (shared with t9_scan.hip) */

/* the operator's identity in the (encoded) table domain */
inline u64 ident_of(int op) {
    return op == T9_OP_MIN ? ~0ull : 0ull;
}

template <int OP>
__device__ inline void t9_comb(u64* p, u64 v) {
    if (OP == T9_OP_SUM)
        atomicAdd((unsigned long long*)p, (unsigned long long)v);
    else if (OP == T9_OP_MIN)
        atomicMin((unsigned long long*)p, (unsigned long long)v);
    else
        atomicMax((unsigned long long*)p, (unsigned long long)v);
}

} // namespace

/* ---------------------------- u64-key table ------------------------- */

__global__ __launch_bounds__(256) void k_reduce_init_op(
    u64* __restrict__ t, u64 cap, u64 ident) {
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i <= cap; i += stride) {
        t[2 * i] = (i == cap) ? 0 : T9_EMPTY;  /* aux slot: occurrences */
        t[2 * i + 1] = ident;
    }
}

/* global-table insert shared by the cold path and the flush */
template <int OP, bool READFIRST>
__device__ inline void t9_g64_insert(u64* __restrict__ t, u64 cap, u64 h,
                                     u64 k, u64 v, u32* __restrict__ err) {
    u64 slot = h & (cap - 1);
    u64 probes = 0;
    for (;;) {
        u64 prev;
        if (READFIRST) {
            prev = __atomic_load_n((unsigned long long*)&t[2 * slot],
                                   __ATOMIC_RELAXED);
            if (prev == T9_EMPTY)
                prev = atomicCAS((unsigned long long*)&t[2 * slot],
                                 (unsigned long long)T9_EMPTY,
                                 (unsigned long long)k);
        }
        else {
            prev = atomicCAS((unsigned long long*)&t[2 * slot],
                             (unsigned long long)T9_EMPTY,
                             (unsigned long long)k);
        }
        if (prev == T9_EMPTY || prev == k) {
            t9_comb<OP>(&t[2 * slot + 1], v);
            return;
        }
        slot = (slot + 1) & (cap - 1);
        if (++probes > cap) {
            atomicExch(err, 1u);
            return;
        }
    }
}

/* LDS-accumulated build, as k_reduce_build_lds: a per-block LDS table
 * absorbs the hot keys, misses go straight to the global table, the block
 * flushes once at the end. Every combine — LDS accumulate, cold insert,
 * flush, aux sentinel slot — applies OP to the encoded value. */
template <int OP, int SLOTS, bool READFIRST>
__global__ __launch_bounds__(256) void k_reduce_build_op(
    const u64* __restrict__ keys, const u64* __restrict__ vals, u64 n,
    u64* __restrict__ t, u64 cap, u64 salt, int vtype, u64 ident,
    u32* __restrict__ err) {
    __shared__ u64 lk[SLOTS];
    __shared__ u64 lv[SLOTS];
    const u32 tid = threadIdx.x;
    for (u32 s = tid; s < (u32)SLOTS; s += 256) {
        lk[s] = T9_EMPTY;
        lv[s] = ident;
    }
    __syncthreads();

    const u64 gsz = (u64)gridDim.x * 256;
    for (u64 base = (u64)blockIdx.x * 256; base < n; base += gsz) {
        const u64 i = base + tid;
        if (i >= n) continue;
        const u64 k = keys[i];
        const u64 v = t9_enc(vals[i], OP, vtype);
        if (k == T9_EMPTY) {
            /* the aux slot counts occurrences with an add and combines
             * the value with the operator */
            atomicAdd((unsigned long long*)&t[2 * cap], 1ull);
            t9_comb<OP>(&t[2 * cap + 1], v);
            continue;
        }
        const u64 h = t9_hash128to64(salt, k);
        u32 ls = (u32)(h >> 48) & (SLOTS - 1);
        bool done = false;
        for (int p = 0; p < 4; ++p) {
            u64 prev;
            if (READFIRST) {
                prev = lk[ls];
                if (prev == T9_EMPTY)
                    prev = atomicCAS((unsigned long long*)&lk[ls],
                                     (unsigned long long)T9_EMPTY,
                                     (unsigned long long)k);
            }
            else {
                prev = atomicCAS((unsigned long long*)&lk[ls],
                                 (unsigned long long)T9_EMPTY,
                                 (unsigned long long)k);
            }
            if (prev == T9_EMPTY || prev == k) {
                t9_comb<OP>(&lv[ls], v);
                done = true;
                break;
            }
            ls = (ls + 1) & (SLOTS - 1);
        }
        if (!done) t9_g64_insert<OP, READFIRST>(t, cap, h, k, v, err);
    }
    __syncthreads();

    for (u32 s = tid; s < (u32)SLOTS; s += 256) {
        const u64 k = lk[s];
        if (k == T9_EMPTY) continue;
        t9_g64_insert<OP, false>(t, cap, t9_hash128to64(salt, k), k, lv[s],
                                 err);
    }
}

/* drain with block-local aggregation (as k_reduce_drain), decoding the
 * value words */
__global__ __launch_bounds__(256) void k_reduce_drain_op(
    const u64* __restrict__ t, u64 cap, int op, int vtype,
    u64* __restrict__ ok, u64* __restrict__ ov, u64* __restrict__ out_n) {
    __shared__ u32 s_pre[256];
    __shared__ u64 s_base;
    const u32 tid = threadIdx.x;
    const u64 stride = (u64)gridDim.x * 256;
    const u64 gid = (u64)blockIdx.x * 256 + tid;
    u32 mine = 0;
    for (u64 i = gid; i < cap; i += stride)
        if (t[2 * i] != T9_EMPTY) ++mine;
    s_pre[tid] = mine;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        u32 y = (tid >= (u32)off) ? s_pre[tid - off] : 0;
        __syncthreads();
        s_pre[tid] += y;
        __syncthreads();
    }
    if (tid == 255 && s_pre[255])
        s_base = atomicAdd((unsigned long long*)out_n,
                           (unsigned long long)s_pre[255]);
    __syncthreads();
    if (mine) {
        u64 pos = s_base + s_pre[tid] - mine;
        for (u64 i = gid; i < cap; i += stride) {
            if (t[2 * i] != T9_EMPTY) {
                ok[pos] = t[2 * i];
                ov[pos] = t9_dec(t[2 * i + 1], op, vtype);
                ++pos;
            }
        }
    }
    if (gid == 0 && t[2 * cap] > 0) {
        u64 pos = atomicAdd((unsigned long long*)out_n, 1ull);
        ok[pos] = T9_EMPTY;
        ov[pos] = t9_dec(t[2 * cap + 1], op, vtype);
    }
}

/* ------------------------ 128-bit composite key --------------------- *
 * Slot = 3 packed u64 {k1, k2, value}; the 4-u64 stride of
 * T9_R128_STRIDE=4 is not instantiated here and is refused by the host
 * entry points. Claim protocol and probe order are t9_g128_insert's, so
 * t9_reduce128_lookup finds the keys of a table built with any operator. */

__global__ __launch_bounds__(256) void k_reduce128_init_op(
    u64* __restrict__ t, u64 cap, u64 ident) {
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < cap;
         i += stride) {
        t[3 * i] = T9_EMPTY;
        t[3 * i + 1] = T9_EMPTY;
        t[3 * i + 2] = ident;
    }
}

template <int OP, bool READFIRST>
__device__ inline void t9_g128_insert_op(u64* __restrict__ t, u64 cap,
                                         u64 salt, u64 k1, u64 k2, u64 v,
                                         u32* __restrict__ err) {
    u64 slot = t9_hash128to64(salt, k1) & (cap - 1);
    u64 probes = 0;
    for (;;) {
        u64 p1;
        if (READFIRST) {
            p1 = __atomic_load_n((unsigned long long*)&t[3 * slot],
                                 __ATOMIC_RELAXED);
            if (p1 == T9_EMPTY)
                p1 = atomicCAS((unsigned long long*)&t[3 * slot],
                               (unsigned long long)T9_EMPTY,
                               (unsigned long long)k1);
        }
        else {
            p1 = atomicCAS((unsigned long long*)&t[3 * slot],
                           (unsigned long long)T9_EMPTY,
                           (unsigned long long)k1);
        }
        if (p1 == T9_EMPTY || p1 == k1) {
            u64 p2;
            if (READFIRST) {
                p2 = __atomic_load_n((unsigned long long*)&t[3 * slot + 1],
                                     __ATOMIC_RELAXED);
                if (p2 == T9_EMPTY)
                    p2 = atomicCAS((unsigned long long*)&t[3 * slot + 1],
                                   (unsigned long long)T9_EMPTY,
                                   (unsigned long long)k2);
            }
            else {
                p2 = atomicCAS((unsigned long long*)&t[3 * slot + 1],
                               (unsigned long long)T9_EMPTY,
                               (unsigned long long)k2);
            }
            if (p2 == T9_EMPTY || p2 == k2) {
                t9_comb<OP>(&t[3 * slot + 2], v);
                return;
            }
            /* k1 matches, k2 differs: a k1 collision — probe on */
        }
        slot = (slot + 1) & (cap - 1);
        if (++probes > cap) {
            atomicExch(err, 1u);
            return;
        }
    }
}

template <int OP, int SLOTS, bool READFIRST>
__global__ __launch_bounds__(256) void k_reduce128_build_op(
    const u64* __restrict__ k1s, const u64* __restrict__ k2s,
    const u64* __restrict__ vals, u64 n, u64* __restrict__ t, u64 cap,
    u64 salt, int vtype, u64 ident, u32* __restrict__ err) {
    __shared__ u64 lk1[SLOTS];
    __shared__ u64 lk2[SLOTS];
    __shared__ u64 lv[SLOTS];
    const u32 tid = threadIdx.x;
    for (u32 s = tid; s < (u32)SLOTS; s += 256) {
        lk1[s] = T9_EMPTY;
        lk2[s] = T9_EMPTY;
        lv[s] = ident;
    }
    __syncthreads();

    const u64 gsz = (u64)gridDim.x * 256;
    for (u64 base = (u64)blockIdx.x * 256; base < n; base += gsz) {
        const u64 i = base + tid;
        if (i >= n) continue;
        const u64 k1 = k1s[i], k2 = k2s[i];
        /* vals == NULL ("count 1") reaches here only with OP = SUM */
        const u64 v = vals ? t9_enc(vals[i], OP, vtype) : 1;
        const u64 h = t9_hash128to64(salt, k1);
        u32 ls = (u32)(h >> 48) & (SLOTS - 1);
        bool done = false;
        for (int p = 0; p < 4; ++p) {
            u64 p1;
            if (READFIRST) {
                p1 = lk1[ls];
                if (p1 == T9_EMPTY)
                    p1 = atomicCAS((unsigned long long*)&lk1[ls],
                                   (unsigned long long)T9_EMPTY,
                                   (unsigned long long)k1);
            }
            else {
                p1 = atomicCAS((unsigned long long*)&lk1[ls],
                               (unsigned long long)T9_EMPTY,
                               (unsigned long long)k1);
            }
            if (p1 == T9_EMPTY || p1 == k1) {
                u64 p2;
                if (READFIRST) {
                    p2 = lk2[ls];
                    if (p2 == T9_EMPTY)
                        p2 = atomicCAS((unsigned long long*)&lk2[ls],
                                       (unsigned long long)T9_EMPTY,
                                       (unsigned long long)k2);
                }
                else {
                    p2 = atomicCAS((unsigned long long*)&lk2[ls],
                                   (unsigned long long)T9_EMPTY,
                                   (unsigned long long)k2);
                }
                if (p2 == T9_EMPTY || p2 == k2) {
                    t9_comb<OP>(&lv[ls], v);
                    done = true;
                    break;
                }
            }
            ls = (ls + 1) & (SLOTS - 1);
        }
        if (!done)
            t9_g128_insert_op<OP, READFIRST>(t, cap, salt, k1, k2, v, err);
    }
    __syncthreads();

    for (u32 s = tid; s < (u32)SLOTS; s += 256) {
        if (lk1[s] == T9_EMPTY) continue;
        /* a claimed slot whose k2 nobody won still holds the identity
         * and is skipped */
        if (lk2[s] == T9_EMPTY) continue;
        t9_g128_insert_op<OP, READFIRST>(t, cap, salt, lk1[s], lk2[s],
                                         lv[s], err);
    }
}

__global__ __launch_bounds__(256) void k_reduce128_drain_op(
    const u64* __restrict__ t, u64 cap, int op, int vtype,
    u64* __restrict__ ok1, u64* __restrict__ ok2, u64* __restrict__ ov,
    u64* __restrict__ out_n) {
    __shared__ u32 s_pre[256];
    __shared__ u64 s_base;
    const u32 tid = threadIdx.x;
    const u64 stride = (u64)gridDim.x * 256;
    const u64 gid = (u64)blockIdx.x * 256 + tid;
    u32 mine = 0;
    for (u64 i = gid; i < cap; i += stride)
        if (t[3 * i] != T9_EMPTY && t[3 * i + 1] != T9_EMPTY) ++mine;
    s_pre[tid] = mine;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        u32 y = (tid >= (u32)off) ? s_pre[tid - off] : 0;
        __syncthreads();
        s_pre[tid] += y;
        __syncthreads();
    }
    if (tid == 255 && s_pre[255])
        s_base = atomicAdd((unsigned long long*)out_n,
                           (unsigned long long)s_pre[255]);
    __syncthreads();
    if (mine) {
        u64 pos = s_base + s_pre[tid] - mine;
        for (u64 i = gid; i < cap; i += stride) {
            if (t[3 * i] != T9_EMPTY && t[3 * i + 1] != T9_EMPTY) {
                ok1[pos] = t[3 * i];
                ok2[pos] = t[3 * i + 1];
                ov[pos] = t9_dec(t[3 * i + 2], op, vtype);
                ++pos;
            }
        }
    }
}

/* ------------------------------ by index ---------------------------- *
 * dense[i] = fold of the values whose key is begin + i, or `neutral` if no
 * item has that key — the neutral element is not folded in
 * (core/reduce_by_index_post_phase.hpp:150-172). "Untouched" is its own
 * record, a bitmap in the workspace: an index whose only values equal the
 * operator's identity still yields that value. */

__global__ __launch_bounds__(256) void k_by_index_init_op(
    u64* __restrict__ dense, u64 size, u64 ident, u32* __restrict__ touched,
    u64 words) {
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < size;
         i += stride) {
        dense[i] = ident;
        if (i < words) touched[i] = 0;
    }
}

template <int OP>
__global__ __launch_bounds__(256) void k_by_index_op(
    const u64* __restrict__ keys, const u64* __restrict__ vals, u64 n,
    u64 begin, u64 size, int vtype, u64* __restrict__ dense,
    u32* __restrict__ touched, u32* __restrict__ err) {
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const u64 k = keys[i];
        if (k < begin || k - begin >= size) {
            atomicExch(err, 1u);
            continue;
        }
        const u64 d = k - begin;
        t9_comb<OP>(&dense[d], t9_enc(vals[i], OP, vtype));
        const u32 bit = 1u << (d & 31);
        /* a set bit never clears: skip the atomic once it reads set */
        if (!(__atomic_load_n(&touched[d >> 5], __ATOMIC_RELAXED) & bit))
            atomicOr(&touched[d >> 5], bit);
    }
}

__global__ __launch_bounds__(256) void k_by_index_finish_op(
    u64* __restrict__ dense, u64 size, int op, int vtype, u64 neutral,
    const u32* __restrict__ touched) {
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < size;
         i += stride) {
        const bool hit = (touched[i >> 5] >> (i & 31)) & 1u;
        dense[i] = hit ? t9_dec(dense[i], op, vtype) : neutral;
    }
}

namespace {
u32 grid_for(u64 work) {
    u64 want = (work + 255) / 256;
    return (u32)((want < 4096) ? (want ? want : 1) : 4096);
}
bool is_pow2(u64 x) { return x && !(x & (x - 1)); }
bool op_ok(int op, int vtype) {
    if (op < T9_OP_SUM || op > T9_OP_MAX) return false;
    if (vtype < T9_VAL_U64 || vtype > T9_VAL_F64) return false;
    /* a floating atomic sum depends on arrival order */
    return !(op == T9_OP_SUM && vtype == T9_VAL_F64);
}
/* T9_REDUCE_GRID; 0 = derive from n. false = unusable value. */
bool env_grid(u64 n, u32* grid) {
    const char* ge = getenv("T9_REDUCE_GRID");
    if (ge) {
        const int g = atoi(ge);
        if (g < 1 || g > 65535) return false;
        *grid = (u32)g;
        return true;
    }
    u32 g = grid_for(n);
    *grid = g > 1024 ? 1024 : g;
    return true;
}
bool r128_stride4() {
    const char* e = getenv("T9_R128_STRIDE");
    return e && atoi(e) == 4;
}
} // namespace

#define T9_OP_SWITCH(op, LAUNCH)                                          \
    do {                                                                  \
        if ((op) == T9_OP_SUM) { LAUNCH(T9_OP_SUM); }                     \
        else if ((op) == T9_OP_MIN) { LAUNCH(T9_OP_MIN); }                \
        else { LAUNCH(T9_OP_MAX); }                                       \
    } while (0)

extern "C" {

int t9_reduce_init_op(t9_context* ctx, u64* d_table, u64 cap, int op,
                      int vtype, void* stream) {
    (void)ctx;
    if (!op_ok(op, vtype) || !d_table || !is_pow2(cap)) return T9_EINVAL;
    hipLaunchKernelGGL(k_reduce_init_op, dim3(grid_for(cap + 1)), dim3(256),
                       0, (hipStream_t)stream, d_table, cap, ident_of(op));
    T9_LAUNCH_CHECK();
    return T9_OK;
}

int t9_reduce_build_op(t9_context* ctx, const u64* d_keys,
                       const u64* d_vals, u64 n, u64* d_table, u64 cap,
                       u64 salt, int op, int vtype, u32* d_error,
                       void* stream) {
    (void)ctx;
    if (!op_ok(op, vtype) || !d_table || !d_error || !is_pow2(cap))
        return T9_EINVAL;
    if (n && (!d_keys || !d_vals)) return T9_EINVAL;
    /* Variants: LDS slots 1024 or 4096 (T9_LDS_SLOTS <= 1024 picks 1024,
     * anything else 4096), read-before-CAS on or off
     * (T9_REDUCE_READFIRST). T9_REDUCE_COMBINE and T9_REDUCE_WAVECOMB
     * select legacy schedules this path does not instantiate; the LDS
     * variant serves them — same table layout, same result. */
    const char* se = getenv("T9_LDS_SLOTS");
    const int slots = se ? atoi(se) : 4096;
    u32 grid;
    if (!env_grid(n, &grid)) return T9_EINVAL;
    const char* urf = getenv("T9_REDUCE_READFIRST");
    const bool rf = !(urf && urf[0] == '0');
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_error, 0, 4, s));
    if (n == 0) return T9_OK;
    const u64 ident = ident_of(op);
#define T9_LAUNCH_B(OP)                                                   \
    do {                                                                  \
        if (slots <= 1024 && rf)                                          \
            hipLaunchKernelGGL((k_reduce_build_op<OP, 1024, true>),       \
                               dim3(grid), dim3(256), 0, s, d_keys,       \
                               d_vals, n, d_table, cap, salt, vtype,      \
                               ident, d_error);                           \
        else if (slots <= 1024)                                           \
            hipLaunchKernelGGL((k_reduce_build_op<OP, 1024, false>),      \
                               dim3(grid), dim3(256), 0, s, d_keys,       \
                               d_vals, n, d_table, cap, salt, vtype,      \
                               ident, d_error);                           \
        else if (rf)                                                      \
            hipLaunchKernelGGL((k_reduce_build_op<OP, 4096, true>),       \
                               dim3(grid), dim3(256), 0, s, d_keys,       \
                               d_vals, n, d_table, cap, salt, vtype,      \
                               ident, d_error);                           \
        else                                                              \
            hipLaunchKernelGGL((k_reduce_build_op<OP, 4096, false>),      \
                               dim3(grid), dim3(256), 0, s, d_keys,       \
                               d_vals, n, d_table, cap, salt, vtype,      \
                               ident, d_error);                           \
    } while (0)
    T9_PERF_WRAP(s, "reduce_build_op", T9_OP_SWITCH(op, T9_LAUNCH_B));
#undef T9_LAUNCH_B
    T9_LAUNCH_CHECK();
    return T9_OK;
}

int t9_reduce_drain_op(t9_context* ctx, const u64* d_table, u64 cap, int op,
                       int vtype, u64* d_ok, u64* d_ov, u64* d_out_n,
                       void* stream) {
    (void)ctx;
    if (!op_ok(op, vtype) || !d_table || !d_ok || !d_ov || !d_out_n ||
        !is_pow2(cap))
        return T9_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_out_n, 0, 8, s));
    hipLaunchKernelGGL(k_reduce_drain_op, dim3(grid_for(cap)), dim3(256), 0,
                       s, d_table, cap, op, vtype, d_ok, d_ov, d_out_n);
    T9_LAUNCH_CHECK();
    return T9_OK;
}

int t9_reduce128_init_op(t9_context* ctx, u64* d_table, u64 cap, int op,
                         int vtype, void* stream) {
    (void)ctx;
    if (!op_ok(op, vtype) || !d_table || !is_pow2(cap) || r128_stride4())
        return T9_EINVAL;
    hipLaunchKernelGGL(k_reduce128_init_op, dim3(grid_for(cap)), dim3(256),
                       0, (hipStream_t)stream, d_table, cap, ident_of(op));
    T9_LAUNCH_CHECK();
    return T9_OK;
}

int t9_reduce128_build_op(t9_context* ctx, const u64* d_k1, const u64* d_k2,
                          const u64* d_vals, u64 n, u64* d_table, u64 cap,
                          u64 salt, int op, int vtype, u32* d_error,
                          void* stream) {
    (void)ctx;
    if (!op_ok(op, vtype) || !d_table || !d_error || !is_pow2(cap))
        return T9_EINVAL;
    /* "every pair counts 1" only means something under SUM */
    if (!d_vals && op != T9_OP_SUM) return T9_EINVAL;
    if (n && (!d_k1 || !d_k2)) return T9_EINVAL;
    /* the 4-u64 slot stride has no operator variant: refuse, never mix
     * layouts */
    if (r128_stride4()) return T9_EINVAL;
    /* Variants: LDS slots 1024 or 4096 (T9_LDS128_SLOTS <= 1024 picks
     * 1024, anything else 4096), T9_R128_READFIRST on or off. */
    const char* se = getenv("T9_LDS128_SLOTS");
    const int slots = se ? atoi(se) : 4096;
    u32 grid;
    if (!env_grid(n, &grid)) return T9_EINVAL;
    const char* rfe = getenv("T9_R128_READFIRST");
    const bool rf = !(rfe && rfe[0] == '0');
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_error, 0, 4, s));
    if (n == 0) return T9_OK;
    const u64 ident = ident_of(op);
#define T9_LAUNCH_B(OP)                                                   \
    do {                                                                  \
        if (slots <= 1024 && rf)                                          \
            hipLaunchKernelGGL((k_reduce128_build_op<OP, 1024, true>),    \
                               dim3(grid), dim3(256), 0, s, d_k1, d_k2,   \
                               d_vals, n, d_table, cap, salt, vtype,      \
                               ident, d_error);                           \
        else if (slots <= 1024)                                           \
            hipLaunchKernelGGL((k_reduce128_build_op<OP, 1024, false>),   \
                               dim3(grid), dim3(256), 0, s, d_k1, d_k2,   \
                               d_vals, n, d_table, cap, salt, vtype,      \
                               ident, d_error);                           \
        else if (rf)                                                      \
            hipLaunchKernelGGL((k_reduce128_build_op<OP, 4096, true>),    \
                               dim3(grid), dim3(256), 0, s, d_k1, d_k2,   \
                               d_vals, n, d_table, cap, salt, vtype,      \
                               ident, d_error);                           \
        else                                                              \
            hipLaunchKernelGGL((k_reduce128_build_op<OP, 4096, false>),   \
                               dim3(grid), dim3(256), 0, s, d_k1, d_k2,   \
                               d_vals, n, d_table, cap, salt, vtype,      \
                               ident, d_error);                           \
    } while (0)
    T9_PERF_WRAP(s, "reduce_build_op", T9_OP_SWITCH(op, T9_LAUNCH_B));
#undef T9_LAUNCH_B
    T9_LAUNCH_CHECK();
    return T9_OK;
}

int t9_reduce128_drain_op(t9_context* ctx, const u64* d_table, u64 cap,
                          int op, int vtype, u64* d_ok1, u64* d_ok2,
                          u64* d_ov, u64* d_out_n, void* stream) {
    (void)ctx;
    if (!op_ok(op, vtype) || !d_table || !d_ok1 || !d_ok2 || !d_ov ||
        !d_out_n || !is_pow2(cap) || r128_stride4())
        return T9_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_out_n, 0, 8, s));
    hipLaunchKernelGGL(k_reduce128_drain_op, dim3(grid_for(cap)), dim3(256),
                       0, s, d_table, cap, op, vtype, d_ok1, d_ok2, d_ov,
                       d_out_n);
    T9_LAUNCH_CHECK();
    return T9_OK;
}

/* touched bitmap: one bit per index, u32 words, 256-byte rounded */
u64 t9_reduce_by_index_op_workspace(u64 size) {
    return t9_align256(t9_ceil_div(size, 32) * 4 + 4);
}

int t9_reduce_by_index_op(t9_context* ctx, const u64* d_keys,
                          const u64* d_vals, u64 n, u64 begin, u64 size,
                          int op, int vtype, u64 neutral, u64* d_dense,
                          u32* d_error, void* d_workspace, void* stream) {
    (void)ctx;
    if (!op_ok(op, vtype) || !d_dense || !d_error || !d_workspace ||
        size == 0)
        return T9_EINVAL;
    if (n && (!d_keys || !d_vals)) return T9_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    u32* touched = (u32*)d_workspace;
    const u64 words = t9_ceil_div(size, 32);
    HIP_TRY(hipMemsetAsync(d_error, 0, 4, s));
    hipLaunchKernelGGL(k_by_index_init_op, dim3(grid_for(size)), dim3(256),
                       0, s, d_dense, size, ident_of(op), touched, words);
    if (n) {
#define T9_LAUNCH_B(OP)                                                   \
    hipLaunchKernelGGL((k_by_index_op<OP>), dim3(grid_for(n)), dim3(256),  \
                       0, s, d_keys, d_vals, n, begin, size, vtype,       \
                       d_dense, touched, d_error)
        T9_OP_SWITCH(op, T9_LAUNCH_B);
#undef T9_LAUNCH_B
    }
    hipLaunchKernelGGL(k_by_index_finish_op, dim3(grid_for(size)),
                       dim3(256), 0, s, d_dense, size, op, vtype, neutral,
                       touched);
    T9_LAUNCH_CHECK();
    return T9_OK;
}

} /* extern "C" */
