/* t9_join.hip — InnerJoin on the device: sort-merge join of two u64 key
 * arrays with a load-balanced emit, gfx950.
 *
 * The reference's InnerJoin (api/inner_join.hpp:213-287) orders both sides
 * by key, advances two pullers in step and sends the cartesian product of
 * every pair of equal-key runs through the join function. Here the result
 * is the list of index pairs (i, j) with lkeys[i] == rkeys[j], ordered by
 * key (unsigned), then i, then j; payloads are the caller's business
 * (t9_gather_records on the two index arrays).
 *
 * t9_join_count:
 *   1. each side: keys copied next to an iota (t9_extract_key64_le on
 *      8-byte "records") and sorted stably as (key, index) pairs
 *      (t9_sort_pairs_u64_u32) -> LK/LI, RK/RI. Stability is what orders i
 *      and j inside a key.
 *   2. k_join_bounds: one block per tile of JOIN_LT sorted left keys. Two
 *      block-wide searches bracket the slice of RK that can match the tile
 *      (lower bound of the first key, upper bound of the last); a slice of
 *      at most JOIN_SK keys is staged in LDS with 16-byte loads and every
 *      lane searches there (binary search for the lower bound, a galloping
 *      one from it for the upper), a longer one is searched in global memory.
 *      Per left element: lo (u32, first match in RK) and cnt (u64).
 *   3. t9_scan_u64, exclusive SUM over cnt -> off, and the total.
 *
 * t9_join_emit: k_join_emit divides the work by OUTPUT POSITION. A block
 * owns JOIN_OT consecutive positions [p0, p1). Two searches in `off` give
 * the left span [i0, i1) whose groups meet the tile; the block streams that
 * span once, coalesced, and every element with cnt > 0 drops its (lo, LI)
 * into the LDS slot of the tile position where its group begins (such
 * elements have distinct off, so every slot has one writer; zero-count
 * elements are skipped, so a run of them of any length costs reads and no
 * LDS). A max-scan over the slot numbers then tells every position the
 * slot its group started at, and
 *     out_left[p]  = LI[i]
 *     out_right[p] = RI[lo[i] + (p - off[i])]
 * follow from LDS alone; a lane owns four consecutive positions and stores
 * 16 bytes to each output. One hot left element is spread over as many blocks
 * as its rows need; no lane loops over a group.
 *
 * No atomics, no block waits on another, nothing spins; every result is a
 * deterministic function of the inputs.
 */

#include "t9_common.h"
#include "thrill_amd.h"

#include <cstdlib>

#define JOIN_LT 2048u   /* sorted left keys per block of k_join_bounds */
#define JOIN_SK 4096u   /* most right keys staged in LDS per block */
#define JOIN_OT 2048u   /* output positions per block of k_join_emit */

namespace {

/* First index in [0, n) whose element is > key (UPPER) or >= key (lower
 * bound), n if there is none; a sorted. The 64 lanes of a wave probe 64
 * evenly spaced elements per step, so 2^32 elements take 6 dependent loads
 * instead of 32. Every lane of the wave must call it with the same
 * arguments; every lane gets the result. */
template <bool UPPER>
__device__ __forceinline__ u64 jn_wave_bound(const u64* __restrict__ a,
                                             u64 n, u64 key, u32 lane) {
    u64 lo = 0, hi = n;
    while (hi > lo) {
        const u64 step = (hi - lo + 63) / 64;
        const u64 idx = lo + (u64)lane * step;
        bool before = false;   /* a[idx] lies before the bound */
        if (idx < hi) {
            const u64 v = a[idx];
            before = UPPER ? v <= key : v < key;
        }
        /* a is sorted and the valid probes are a prefix of the lanes, so
         * the lanes with `before` are a prefix too */
        const u32 c = (u32)__popcll(__ballot(before));
        if (c == 0) {
            hi = lo;
        }
        else {
            const u64 nhi = lo + (u64)c * step;
            lo = lo + (u64)(c - 1) * step + 1;
            if (nhi < hi) hi = nhi;
        }
    }
    return lo;
}

/* per-lane binary search of s[b, e): first index whose element is >= key
 * (or > key with UPPER) */
template <bool UPPER>
__device__ __forceinline__ u32 jn_bound(const u64* s, u32 b, u32 e,
                                        u64 key) {
    while (b < e) {
        const u32 m = b + ((e - b) >> 1);
        const u64 v = s[m];
        if (UPPER ? v <= key : v < key) b = m + 1;
        else e = m;
    }
    return b;
}
template <bool UPPER>
__device__ __forceinline__ u64 jn_bound64(const u64* __restrict__ a, u64 b,
                                          u64 e, u64 key) {
    while (b < e) {
        const u64 m = b + ((e - b) >> 1);
        const u64 v = a[m];
        if (UPPER ? v <= key : v < key) b = m + 1;
        else e = m;
    }
    return b;
}

/* Upper bound of key in s[b, e) when s[b-1] < key <= s[b] is known (b is
 * key's lower bound): probe b, b+2, b+6, … with doubling steps until an
 * element is > key, then a binary search between the last two probes. A
 * key with c equal elements takes about 2 log2(c) + 1 probes instead of
 * log2(e - b): one probe for no match, three for a single one. */
__device__ __forceinline__ u32 jn_upper_gallop(const u64* s, u32 b, u32 e,
                                               u64 key) {
    u32 step = 1;
    for (;;) {
        const u32 probe = b + step - 1;
        if (probe >= e) break;
        if (s[probe] > key) {
            e = probe;
            break;
        }
        b = probe + 1;
        step <<= 1;
    }
    return jn_bound<true>(s, b, e, key);
}

__device__ __forceinline__ u32 jn_wave_max_scan(u32 v, u32 lane) {
#pragma unroll
    for (u32 o = 1; o < 64; o <<= 1) {
        const u32 y = __shfl_up(v, o, 64);
        if (lane >= o && y > v) v = y;
    }
    return v;
}

} // namespace

/* Stage 2. lk[0, nl) and rk[0, nr) sorted; rk's allocation is a whole
 * number of 16-byte words (the workspace rounds it), so the 16-byte load
 * that holds rk[nr-1] stays inside it. */
template <bool GALLOP>
__global__ __launch_bounds__(256) void k_join_bounds(
    const u64* __restrict__ lk, u64 nl, const u64* __restrict__ rk, u64 nr,
    u32* __restrict__ lo_out, u64* __restrict__ cnt_out) {
    __shared__ __attribute__((aligned(16))) u64 s_rk[JOIN_SK + 2];
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u64 t0 = (u64)blockIdx.x * JOIN_LT;
    if (t0 >= nl) return;
    const u64 t1 = t0 + JOIN_LT < nl ? t0 + JOIN_LT : nl;
    /* the slice of rk that can match this tile */
    const u64 r0 = jn_wave_bound<false>(rk, nr, lk[t0], lane);
    const u64 r1 = jn_wave_bound<true>(rk, nr, lk[t1 - 1], lane);
    const u64 slice = r1 - r0;   /* r1 >= r0: lk[t0] <= lk[t1-1] */
    if (slice <= JOIN_SK) {      /* block-uniform */
        /* 16-byte loads from the even index at or below r0 */
        const u64 a0 = r0 & ~1ull;
        const u32 skip = (u32)(r0 - a0);
        const u32 pairs = (u32)((r1 - a0 + 1) >> 1);   /* <= SK/2 + 1 */
        for (u32 q = tid; q < pairs; q += 256)
            *(ulonglong2*)(s_rk + 2 * q) =
                *(const ulonglong2*)(rk + a0 + 2 * (u64)q);
        __syncthreads();
        const u64* s = s_rk + skip;
        const u32 sn = (u32)slice;
        for (u64 i = t0 + tid; i < t1; i += 256) {
            const u64 k = lk[i];
            const u32 b = jn_bound<false>(s, 0, sn, k);
            const u32 e = GALLOP ? jn_upper_gallop(s, b, sn, k)
                                 : jn_bound<true>(s, b, sn, k);
            lo_out[i] = (u32)(r0 + b);
            cnt_out[i] = (u64)(e - b);
        }
    }
    else {
        for (u64 i = t0 + tid; i < t1; i += 256) {
            const u64 k = lk[i];
            const u64 b = jn_bound64<false>(rk, r0, r1, k);
            const u64 e = jn_bound64<true>(rk, b, r1, k);
            lo_out[i] = (u32)b;
            cnt_out[i] = e - b;
        }
    }
}

/* Emit. off = exclusive scan of cnt over [0, nl); *total_p = its total.
 * Writes positions [0, min(n_out, total)) of out_left / out_right. */
template <bool V4>
__global__ __launch_bounds__(256) void k_join_emit(
    const u64* __restrict__ off, const u64* __restrict__ cnt,
    const u32* __restrict__ lo, const u32* __restrict__ li,
    const u32* __restrict__ ri, u64 nl, const u64* __restrict__ total_p,
    u64 n_out, u32* __restrict__ out_left, u32* __restrict__ out_right) {
    constexpr u32 R = JOIN_OT / 256;
    /* slot number where a group starts */
    __shared__ __attribute__((aligned(16))) u32 s_q[JOIN_OT];
    __shared__ u32 s_lo[JOIN_OT];   /* first right row of that group here */
    __shared__ u32 s_li[JOIN_OT];   /* its left index */
    __shared__ u32 s_tot[R * 4];
    const u32 tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const u64 total = *total_p;
    const u64 lim = n_out < total ? n_out : total;
    const u64 p0 = (u64)blockIdx.x * JOIN_OT;
    if (p0 >= lim) return;   /* block-uniform */
    const u64 p1 = p0 + JOIN_OT < lim ? p0 + JOIN_OT : lim;
    /* the left span whose groups meet [p0, p1): i0 is the last element
     * with off <= p0 — it has cnt > 0, since the next off is > p0 —, and
     * i1 is one past the last with off <= p1-1 */
    const u64 i0 = jn_wave_bound<true>(off, nl, p0, lane) - 1;
    const u64 i1 = jn_wave_bound<true>(off, nl, p1 - 1, lane);
#pragma unroll
    for (u32 r = 0; r < R; ++r) s_q[r * 256 + tid] = 0;
    __syncthreads();
    for (u64 i = i0 + tid; i < i1; i += 256) {
        const u64 c = cnt[i];
        if (c == 0) continue;
        const u64 o = off[i];
        /* o < p0 only for i0, whose group began in an earlier tile: slot 0
         * takes it from the row that falls on p0 */
        const u32 q = o > p0 ? (u32)(o - p0) : 0u;
        const u32 adv = o < p0 ? (u32)(p0 - o) : 0u;
        s_q[q] = q;
        s_lo[q] = lo[i] + adv;
        s_li[q] = li[i];
    }
    __syncthreads();
    /* inclusive max-scan of s_q: position t learns the slot of its group */
    if (V4) {
        /* a lane owns 4 consecutive positions: 16-byte LDS reads and
         * 16-byte stores */
        constexpr u32 R4 = JOIN_OT / 1024;
        u32 a[R4][4], ex[R4];
#pragma unroll
        for (u32 r = 0; r < R4; ++r) {
            const uint4 m = *(const uint4*)(s_q + r * 1024 + tid * 4);
            a[r][0] = m.x;
            a[r][1] = m.y > a[r][0] ? m.y : a[r][0];
            a[r][2] = m.z > a[r][1] ? m.z : a[r][1];
            a[r][3] = m.w > a[r][2] ? m.w : a[r][2];
            const u32 sc = jn_wave_max_scan(a[r][3], lane);
            const u32 up = __shfl_up(sc, 1, 64);
            ex[r] = lane ? up : 0u;
            if (lane == 63) s_tot[r * 4 + w] = sc;
        }
        __syncthreads();
        u32 run = 0;
#pragma unroll
        for (u32 r = 0; r < R4; ++r) {
            u32 pre = run;
#pragma unroll
            for (u32 k = 0; k < 4; ++k) {
                const u32 t = s_tot[r * 4 + k];
                if (k < w && t > pre) pre = t;
                if (t > run) run = t;
            }
            if (ex[r] > pre) pre = ex[r];
            const u32 t0 = r * 1024 + tid * 4;
            const u64 p = p0 + t0;
            u32 ol[4], orr[4];
#pragma unroll
            for (u32 j = 0; j < 4; ++j) {
                const u32 q = pre > a[r][j] ? pre : a[r][j];
                ol[j] = 0;
                orr[j] = 0;
                if (p + j < p1) {
                    ol[j] = s_li[q];
                    orr[j] = ri[s_lo[q] + (t0 + j - q)];
                }
            }
            if (p + 4 <= p1) {   /* p is a multiple of 4 */
                *(uint4*)(out_left + p) =
                    make_uint4(ol[0], ol[1], ol[2], ol[3]);
                *(uint4*)(out_right + p) =
                    make_uint4(orr[0], orr[1], orr[2], orr[3]);
            }
            else {
#pragma unroll
                for (u32 j = 0; j < 4; ++j)
                    if (p + j < p1) {
                        out_left[p + j] = ol[j];
                        out_right[p + j] = orr[j];
                    }
            }
        }
        return;
    }
    u32 v[R];
#pragma unroll
    for (u32 r = 0; r < R; ++r) {
        v[r] = jn_wave_max_scan(s_q[r * 256 + tid], lane);
        if (lane == 63) s_tot[r * 4 + w] = v[r];
    }
    __syncthreads();
    u32 run = 0;
#pragma unroll
    for (u32 r = 0; r < R; ++r) {
        u32 pre = run;
#pragma unroll
        for (u32 k = 0; k < 4; ++k) {
            const u32 t = s_tot[r * 4 + k];
            if (k < w && t > pre) pre = t;
            if (t > run) run = t;
        }
        const u32 q = pre > v[r] ? pre : v[r];
        const u32 t = r * 256 + tid;
        const u64 p = p0 + t;
        if (p < p1) {
            out_left[p] = s_li[q];
            out_right[p] = ri[s_lo[q] + (t - q)];
        }
    }
}

namespace {

/* A/B knobs, read on every call (DESIGN.md "Join"): T9_JOIN_GALLOP=0 turns
 * the galloping upper bound of k_join_bounds into a plain binary search,
 * T9_JOIN_EMIT_V4=0 makes k_join_emit write one position per lane and
 * round instead of four. The results are the same. */
bool knob_on(const char* name) {
    const char* e = getenv(name);
    return !(e && e[0] == '0');
}

struct JoinWs {
    u64* head;   /* [0] = total */
    u64 *lk, *rk, *cnt, *off;
    u32 *li, *ri, *lo;
    void *sort_ws, *scan_ws;
    u64 bytes;
};

/* pure host arithmetic: carve(nullptr, ...) sizes the workspace */
JoinWs carve(void* ws, u64 nl, u64 nr) {
    JoinWs w;
    u8* p = (u8*)ws;
    u64 o = 0;
    auto take = [&](u64 bytes) {
        u8* q = p + o;
        o += t9_align256(bytes);
        return (void*)q;
    };
    w.head = (u64*)take(256);
    w.lk = (u64*)take(nl * 8);
    w.rk = (u64*)take(nr * 8);
    w.cnt = (u64*)take(nl * 8);
    w.off = (u64*)take(nl * 8);
    w.li = (u32*)take(nl * 4);
    w.ri = (u32*)take(nr * 4);
    w.lo = (u32*)take(nl * 4);
    const u64 sl = t9_sort_pairs_workspace(nl);
    const u64 sr = t9_sort_pairs_workspace(nr);
    w.sort_ws = take(sl > sr ? sl : sr);
    w.scan_ws = take(t9_scan_workspace(nl));
    w.bytes = o;
    return w;
}

} // namespace

extern "C" {

void t9_join_geometry(uint32_t* left_tile, uint32_t* out_tile,
                      uint32_t* stage_keys) {
    if (left_tile) *left_tile = JOIN_LT;
    if (out_tile) *out_tile = JOIN_OT;
    if (stage_keys) *stage_keys = JOIN_SK;
}

u64 t9_join_workspace(u64 n_left, u64 n_right) {
    return carve(nullptr, n_left, n_right).bytes;
}

int t9_join_count(t9_context* ctx, const u64* d_lkeys, u64 n_left,
                  const u64* d_rkeys, u64 n_right, u64* total,
                  void* d_workspace, void* stream) {
    if (n_left >= (1ull << 32) || n_right >= (1ull << 32)) return T9_EINVAL;
    if (!total) return T9_EINVAL;
    if ((n_left && !d_lkeys) || (n_right && !d_rkeys)) return T9_EINVAL;
    /* its size is never zero; the kernels read it in 16-byte words */
    if (!d_workspace || ((uintptr_t)d_workspace & 15)) return T9_EINVAL;
    *total = 0;
    if (n_left == 0 || n_right == 0) return T9_OK;
    hipStream_t s = (hipStream_t)stream;
    const JoinWs w = carve(d_workspace, n_left, n_right);
    int rc;
    /* (key, iota) of each side, sorted stably by key */
    if ((rc = t9_extract_key64_le(ctx, (const u8*)d_lkeys, n_left, 8, 0,
                                  w.lk, w.li, stream)) != T9_OK)
        return rc;
    if ((rc = t9_sort_pairs_u64_u32(ctx, w.lk, w.li, n_left, w.sort_ws,
                                    stream)) != T9_OK)
        return rc;
    if ((rc = t9_extract_key64_le(ctx, (const u8*)d_rkeys, n_right, 8, 0,
                                  w.rk, w.ri, stream)) != T9_OK)
        return rc;
    if ((rc = t9_sort_pairs_u64_u32(ctx, w.rk, w.ri, n_right, w.sort_ws,
                                    stream)) != T9_OK)
        return rc;
    const u32 g = (u32)t9_ceil_div(n_left, JOIN_LT);
    if (knob_on("T9_JOIN_GALLOP"))
        T9_PERF_WRAP(s, "join_bounds",
                     hipLaunchKernelGGL(k_join_bounds<true>, dim3(g),
                                        dim3(256), 0, s, w.lk, n_left, w.rk,
                                        n_right, w.lo, w.cnt));
    else
        T9_PERF_WRAP(s, "join_bounds",
                     hipLaunchKernelGGL(k_join_bounds<false>, dim3(g),
                                        dim3(256), 0, s, w.lk, n_left, w.rk,
                                        n_right, w.lo, w.cnt));
    T9_LAUNCH_CHECK();
    if ((rc = t9_scan_u64(ctx, w.cnt, w.off, n_left, T9_OP_SUM, T9_VAL_U64,
                          1, 0, w.head, w.scan_ws, stream)) != T9_OK)
        return rc;
    HIP_TRY(hipMemcpyAsync(total, w.head, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return T9_OK;
}

int t9_join_emit(t9_context* ctx, u64 n_left, u64 n_right,
                 const void* d_workspace, u64 n_out, u32* d_out_left,
                 u32* d_out_right, void* stream) {
    (void)ctx;
    if (n_left >= (1ull << 32) || n_right >= (1ull << 32)) return T9_EINVAL;
    if (!d_workspace || ((uintptr_t)d_workspace & 15)) return T9_EINVAL;
    if (n_out &&(!d_out_left || !d_out_right)) return T9_EINVAL;
    const u64 nb = t9_ceil_div(n_out, JOIN_OT);
    if (nb >= (1ull << 31)) return T9_EINVAL;
    /* an empty side: t9_join_count launched nothing and the result is
     * empty */
    if (n_left == 0 || n_right == 0 || n_out == 0) return T9_OK;
    hipStream_t s = (hipStream_t)stream;
    const JoinWs w = carve(const_cast<void*>(d_workspace), n_left, n_right);
    /* 16-byte stores need 16-byte aligned outputs */
    const bool v4 = knob_on("T9_JOIN_EMIT_V4") &&
                    (((uintptr_t)d_out_left | (uintptr_t)d_out_right) & 15) == 0;
    if (v4)
        T9_PERF_WRAP(s, "join_emit",
                     hipLaunchKernelGGL(k_join_emit<true>, dim3((u32)nb),
                                        dim3(256), 0, s, w.off, w.cnt, w.lo,
                                        w.li, w.ri, n_left, w.head, n_out,
                                        d_out_left, d_out_right));
    else
        T9_PERF_WRAP(s, "join_emit",
                     hipLaunchKernelGGL(k_join_emit<false>, dim3((u32)nb),
                                        dim3(256), 0, s, w.off, w.cnt, w.lo,
                                        w.li, w.ri, n_left, w.head, n_out,
                                        d_out_left, d_out_right));
    T9_LAUNCH_CHECK();
    return T9_OK;
}

} /* extern "C" */
