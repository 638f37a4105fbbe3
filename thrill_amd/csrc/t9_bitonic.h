/* t9_bitonic.h — register/shfl bitonic alternative to k_lds_sort_sub
 * (included by t9_sort_msb.hip; selected with T9_LDS_BITONIC=1).
 *
 * Motivation (profiles/r01_pmc_wavecycle_decomposition.txt): the 6-pass
 * LDS counting sort is 58% wave-parked on its ~38 block barriers with
 * only 4% LDS-conflict stall, so the fix is structural: a bitonic
 * network runs 52 of its 55 compare-exchange stages entirely in
 * registers/crosslane (no barrier, no LDS), leaving only the j>=256
 * stages (3/6/10 for SUBMAX 1024/2048/4096) to stage through LDS.
 *
 * Stability: bitonic networks are not stable, so the network sorts the
 * composite c = (key & mask48) << 12 | pos (pos = load index < 4096).
 * Composites are unique, ties in low-48 resolve to input order — the
 * exact order the stable radix passes produce. The high 16 key bits are
 * shared by every element of a sub-bucket (byte-7 + level-2 digit), so
 * the key is reconstructed as shared_high | (c >> 12) and need not be
 * carried through the network.
 *
 * Element mapping: e = tid*4 + r (4 registers per thread, wave w owns
 * the contiguous run [w*256, (w+1)*256)). CE distance j=1,2: register
 * pair inside the lane; j=4..128: __shfl_xor at lane distance j/4;
 * j>=256: LDS exchange at wave distance j/256.
 * Padding: slots >= ns carry c = ~0 (sinks to the end, never written
 * back); pad-vs-pad CEs may duplicate pad payloads, which is harmless
 * because the composite multiset above ns stays all-max. */
#pragma once
#include "t9_common.h"

/* one compare-exchange against a crosslane partner: both sides compute;
 * take the partner's element iff (mine > partner) == (I am the lower
 * position in an ascending pair). Composites are unique so c == oc
 * cannot occur between live elements. */
__device__ inline void t9_ce_xor(u64& c, u32& v, u32 lanemask, bool lower,
                                 bool asc) {
    const u64 oc = __shfl_xor(c, lanemask);
    const u32 ov = __shfl_xor(v, lanemask);
    if ((c > oc) == (lower == asc)) { c = oc; v = ov; }
}

template <int SUBMAX, int BLOCK, bool HAS_VAL>
__global__ __launch_bounds__(BLOCK, 2) void k_bitonic_sort_sub(
    u64* __restrict__ keys, u32* __restrict__ vals,
    const u32* __restrict__ sub_start, const u32* __restrict__ sub_n) {
    constexpr int E = SUBMAX / BLOCK;        /* 4 */
    static_assert(E == 4, "mapping assumes 4 elements per thread");
    __shared__ u64 s_c[SUBMAX];
    __shared__ u32 s_v[HAS_VAL ? SUBMAX : 1];
    __shared__ u32 s_differ;

    const u32 sb = blockIdx.x;
    const u32 ns = sub_n[sb];
    if (ns <= 1 || ns > (u32)SUBMAX) return;
    const u32 gbase = sub_start[sb];
    const u32 tid = threadIdx.x, lane = tid & 63;

    if (tid == 0) s_differ = 0;
    __syncthreads();

    const u64 mask48 = 0x0000FFFFFFFFFFFFull;
    const u64 high16 = keys[gbase] & ~mask48;
    const u64 ref48 = keys[gbase] & mask48;

    /* load: 4 contiguous elements per thread -> composite registers */
    u64 c[E];
    u32 v[E];
    u32 differ = 0;
    const u32 e0 = tid * E;
#pragma unroll
    for (int r = 0; r < E; ++r) {
        const u32 i = e0 + r;
        if (i < ns) {
            const u64 k = keys[gbase + i];
            c[r] = ((k & mask48) << 12) | (u64)i;
            if (HAS_VAL) v[r] = vals[gbase + i];
            differ |= ((k & mask48) != ref48);
        } else {
            c[r] = ~0ull;
            if (HAS_VAL) v[r] = 0;
        }
    }
    if (differ) s_differ = 1;
    __syncthreads();
    if (!s_differ) return;   /* all-equal low-48: stable order is in place */

    /* bitonic network over SUBMAX elements — fully unrolled (lk/lj are
     * compile-time constants, so lane masks become immediates and the
     * per-stage branch selection disappears) */
    constexpr int LOG = (SUBMAX == 1024) ? 10 : (SUBMAX == 2048) ? 11 : 12;
#pragma unroll
    for (int lk = 1; lk <= LOG; ++lk) {
        const u32 k = 1u << lk;
#pragma unroll
        for (int lj = lk - 1; lj >= 0; --lj) {
            const u32 j = 1u << lj;
            if (j >= 256) {
                /* cross-wave: stage through LDS */
                __syncthreads();   /* WAR: prior reads of s_c complete */
#pragma unroll
                for (int r = 0; r < E; ++r) {
                    s_c[e0 + r] = c[r];
                    if (HAS_VAL) s_v[e0 + r] = v[r];
                }
                __syncthreads();
#pragma unroll
                for (int r = 0; r < E; ++r) {
                    const u32 e = e0 + r;
                    const u32 p = e ^ j;
                    const u64 oc = s_c[p];
                    const bool lower = (e & j) == 0;
                    const bool asc = (e & k) == 0;
                    if ((c[r] > oc) == (lower == asc)) {
                        c[r] = oc;
                        if (HAS_VAL) v[r] = s_v[p];
                    }
                }
            } else if (j >= 4) {
                /* crosslane within the wave: lane distance j/4 */
                const u32 lm = j >> 2;
#pragma unroll
                for (int r = 0; r < E; ++r) {
                    const u32 e = e0 + r;
                    t9_ce_xor(c[r], v[r], lm, (lane & lm) == 0,
                              (e & k) == 0);
                }
            } else {
                /* register pair inside the lane: r ^ j (j = 1 or 2) */
#pragma unroll
                for (int r = 0; r < E; ++r) {
                    const int q = r ^ (int)j;
                    if (q > r) {
                        const bool asc = ((e0 + r) & k) == 0;
                        if ((c[r] > c[q]) == asc) {
                            u64 tc = c[r]; c[r] = c[q]; c[q] = tc;
                            if (HAS_VAL) {
                                u32 tv = v[r]; v[r] = v[q]; v[q] = tv;
                            }
                        }
                    }
                }
            }
        }
    }

    /* write back: reconstruct keys from composites; element e0+r of the
     * sorted order lives in register r of thread tid */
#pragma unroll
    for (int r = 0; r < E; ++r) {
        const u32 i = e0 + r;
        if (i < ns) {
            keys[gbase + i] = high16 | (c[r] >> 12);
            if (HAS_VAL) vals[gbase + i] = v[r];
        }
    }
}

/* ------------------------------------------------------------------ *
 * wave16 blocksort (T9_LDS_WAVE16=1): single-wave block, 16 elements
 * per lane. The in-lane sort is a pure-VALU bitonic network over
 * registers (zero LDS traffic where the radix sort spends 4 of its 6
 * passes), then 6 merge rounds (16->1024) via merge-path splits into
 * LDS: one 16-byte-slot row store per lane, the binary search, and one
 * LDS read per merged element (the two run heads stay in registers).
 * With a 64-thread block every __syncthreads() compiles to a wave-level
 * scheduling barrier (no s_barrier cost). Same stable-composite scheme
 * as k_bitonic_sort_sub above.
 *
 * k_wave16_sort_sub moves its global data through the same LDS buffer:
 * lane t loads and stores positions t + BLOCK * r (contiguous across the
 * wave) and the buffer turns them into 16 contiguous elements per lane
 * and back. Measured at the 10 GiB record sort:
 * 2.37 ms with lane-strided global I/O and a linear LDS image, 0.93 ms
 * now; the swizzle and the single-read merge only pay once the global
 * I/O is coalesced (before that they measured +0.18 ms).
 * ------------------------------------------------------------------ */
typedef unsigned long long t9_u64x2 __attribute__((ext_vector_type(2)));

/* LDS image of the composites: element e lives at lc[t9_w16_phys(e)].
 * Lane-row l = e >> 4 is 8 slots of 16 bytes; slot k of row l is stored at
 * slot k ^ (l & 7) of the same row (no padding, NSORT * 8 bytes). A lane's
 * eight 16-byte row accesses then fall on eight different bank quads within
 * every group of 8 lanes, and the merge's reads, whose lanes sit about 8
 * elements apart, spread over 16 bank pairs instead of 4. The swizzle never
 * splits a 16-byte slot, so a row moves as eight 128-bit accesses. */
__device__ __forceinline__ u32 t9_w16_phys(u32 e) {
    return e ^ (((e >> 4) & 7u) << 1);
}

/* lane `row` <-> its 16 contiguous elements, as 8 swizzled 16-byte slots */
__device__ __forceinline__ void t9_w16_row_store(u64* lc, u32 row,
                                                 const u64 (&c)[16]) {
    /* row * 16 + ((k ^ x) << 1) == (row * 16 + (x << 1)) ^ (k << 1) */
    const u32 base = row * 16 + ((row & 7u) << 1);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        t9_u64x2 v2;
        v2.x = c[2 * k];
        v2.y = c[2 * k + 1];
        *(t9_u64x2*)&lc[base ^ ((u32)k << 1)] = v2;
    }
}

__device__ __forceinline__ void t9_w16_row_load(const u64* lc, u32 row,
                                                u64 (&c)[16]) {
    const u32 base = row * 16 + ((row & 7u) << 1);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const t9_u64x2 v2 = *(const t9_u64x2*)&lc[base ^ ((u32)k << 1)];
        c[2 * k] = v2.x;
        c[2 * k + 1] = v2.y;
    }
}

/* the blocksort of k_wave16_sort_sub (in-lane network + merge rounds) as a
 * function, for k_wave16_sort_gather; k_wave16_sort_sub keeps its own
 * inline copy so that its code stays exactly what was measured. Lane
 * `lane` enters with its 16 contiguous elements in c[] and leaves with
 * elements lane * 16 .. + 15 of the sorted block. lc is scratch (every
 * round starts with a barrier of its own). */
template <int E, int ROUNDS>
__device__ __forceinline__ void t9_w16_blocksort(u64* lc, u32 lane,
                                                 u64 (&c)[E]) {
    const u32 e0 = lane * E;
    /* in-register bitonic sort of the lane's 16 elements (pure VALU) */
#pragma unroll
    for (int lk = 1; lk <= 4; ++lk) {
        const int k = 1 << lk;
#pragma unroll
        for (int lj = lk - 1; lj >= 0; --lj) {
            const int j = 1 << lj;
#pragma unroll
            for (int r = 0; r < E; ++r) {
                const int q = r ^ j;
                if (q > r) {
                    const bool asc = (r & k) == 0;
                    if ((c[r] > c[q]) == asc) {
                        u64 tc = c[r]; c[r] = c[q]; c[q] = tc;
                    }
                }
            }
        }
    }

    /* 6 merge rounds: sorted runs of L pairwise -> 2L via merge-path.
     * Composites are unique, so `<=` against the B run is a stable merge
     * (A-run elements precede equal... equality cannot occur). */
#pragma unroll
    for (int lm = 0; lm < ROUNDS; ++lm) {
        const u32 L = (u32)E << lm;
        __syncthreads();
        t9_w16_row_store(lc, lane, c);
        __syncthreads();
        const u32 pairbase = e0 & ~(2 * L - 1);
        const u32 d = e0 - pairbase;          /* my first output diagonal */
        const u32 ab = pairbase, bb = pairbase + L;   /* run A, run B */
        u32 lo = (d > L) ? d - L : 0;
        u32 hi = (d < L) ? d : L;
        while (lo < hi) {
            const u32 m = (lo + hi) >> 1;
            if (lc[t9_w16_phys(ab + m)] <= lc[t9_w16_phys(bb + d - m - 1)])
                lo = m + 1;
            else hi = m;
        }
        /* both run heads live in registers; each step emits the
         * smaller one and reads only that side's successor. An
         * exhausted run reads as ~0, above every live composite
         * (60 bits) and equal to the pads, which never leave. */
        u32 ia = ab + lo, ib = bb + (d - lo);
        const u32 ea = bb, eb = bb + L;
        /* reads are unconditional at a clamped index and the value is
         * selected afterwards: no divergent branch per step */
        const u64 a0 = lc[t9_w16_phys(ia < ea ? ia : ab)];
        const u64 b0 = lc[t9_w16_phys(ib < eb ? ib : ab)];
        u64 a = (ia < ea) ? a0 : ~0ull;
        u64 b = (ib < eb) ? b0 : ~0ull;
#pragma unroll
        for (int r = 0; r < E; ++r) {
            const bool ta = a <= b;
            c[r] = ta ? a : b;
            if (r + 1 < E) {
                ia += ta ? 1u : 0u;
                ib += ta ? 0u : 1u;
                const u32 nx = ta ? ia : ib;
                const bool in = nx < (ta ? ea : eb);
                const u64 ld = lc[t9_w16_phys(in ? nx : ab)];
                const u64 nv = in ? ld : ~0ull;
                a = ta ? nv : a;
                b = ta ? b : nv;
            }
        }
    }
}

/* REC (record sort only; needs HAS_VAL): the block also counts its
 * equal-key neighbours into *ntied — the number k_count_tied would find in
 * this sub-bucket; ties cannot cross sub-buckets, whose top key bits
 * differ — and writes its sorted KEYS back only if it found one.
 * Invariant the record sort relies on: a sub-bucket whose keys were not
 * written still holds its own keys, all distinct, in unsorted order, so no
 * two neighbours in it are equal (k_tie_flags flags nothing there) and
 * every later reader of the key array touches tied positions only, which
 * lie in written sub-buckets. The values are always written. The public
 * pair and key sorts instantiate REC = false and get fully sorted keys. */
template <int NSORT, int BLOCK, bool HAS_VAL, bool REC>
__global__ __launch_bounds__(BLOCK, 2) void k_wave16_sort_sub(
    u64* __restrict__ keys, u32* __restrict__ vals,
    const u32* __restrict__ sub_start, const u32* __restrict__ sub_n,
    u32* __restrict__ ntied) {
    constexpr int E = NSORT / BLOCK;
    static_assert(E == 16, "wave16 mapping: 16 elements per lane");
    static_assert(HAS_VAL || !REC, "the tie count rides the pair sort");
    constexpr int ROUNDS = (NSORT == 1024) ? 6 : (NSORT == 2048) ? 7 : 8;
    __shared__ __attribute__((aligned(16))) u64 lc[NSORT];
    __shared__ u32 s_differ;
    __shared__ u32 s_ntie;

    const u32 sb = blockIdx.x;
    const u32 ns = sub_n[sb];
    if (ns <= 1 || ns > (u32)NSORT) return;
    const u32 gbase = sub_start[sb];
    const u32 lane = threadIdx.x;   /* block-level thread id */
    const u32 e0 = lane * E;

    if (lane == 0) { s_differ = 0; s_ntie = 0; }
    __syncthreads();

    const u64 mask48 = 0x0000FFFFFFFFFFFFull;
    const u64 high16 = keys[gbase] & ~mask48;
    const u64 ref48 = keys[gbase] & mask48;

    /* the composite embeds the ORIGINAL position (low 12 bits), so the
     * value array never travels through the sort at all — it is
     * re-gathered from global at writeback (r2: removing the u32 lv LDS
     * array and the v[] registers raises occupancy, the measured
     * limiter of this barrier-parked kernel) */
    u64 c[E];
    u32 differ = 0;
    /* block-uniform bases: the per-lane part of every global address is a
     * 32-bit offset below NSORT elements */
    u64* const kb = keys + gbase;
    u32* const vb = HAS_VAL ? vals + gbase : nullptr;
    /* coalesced load (lane t takes positions t + BLOCK * r), staged
     * through lc so that each lane then owns 16 contiguous elements */
#pragma unroll
    for (int r = 0; r < E; ++r) {
        const u32 p = lane + (u32)BLOCK * r;
        u64 cc = ~0ull;
        if (p < ns) {
            const u64 k = kb[p];
            cc = ((k & mask48) << 12) | (u64)p;
            differ |= ((k & mask48) != ref48);
        }
        lc[t9_w16_phys(p)] = cc;
    }
    if (differ) s_differ = 1;
    __syncthreads();
    if (!s_differ) {
        /* all keys equal: in stable order as they lie, ns - 1 ties */
        if (REC && lane == 0) atomicAdd(ntied, ns - 1);
        return;
    }
    t9_w16_row_load(lc, lane, c);

    /* in-register bitonic sort of the lane's 16 elements (pure VALU) */
#pragma unroll
    for (int lk = 1; lk <= 4; ++lk) {
        const int k = 1 << lk;
#pragma unroll
        for (int lj = lk - 1; lj >= 0; --lj) {
            const int j = 1 << lj;
#pragma unroll
            for (int r = 0; r < E; ++r) {
                const int q = r ^ j;
                if (q > r) {
                    const bool asc = (r & k) == 0;
                    if ((c[r] > c[q]) == asc) {
                        u64 tc = c[r]; c[r] = c[q]; c[q] = tc;
                    }
                }
            }
        }
    }

    /* 6 merge rounds: sorted runs of L pairwise -> 2L via merge-path.
     * Composites are unique, so `<=` against the B run is a stable merge
     * (A-run elements precede equal... equality cannot occur). */
#pragma unroll
    for (int lm = 0; lm < ROUNDS; ++lm) {
        const u32 L = (u32)E << lm;
        __syncthreads();
        t9_w16_row_store(lc, lane, c);
        __syncthreads();
        const u32 pairbase = e0 & ~(2 * L - 1);
        const u32 d = e0 - pairbase;          /* my first output diagonal */
        const u32 ab = pairbase, bb = pairbase + L;   /* run A, run B */
        u32 lo = (d > L) ? d - L : 0;
        u32 hi = (d < L) ? d : L;
        while (lo < hi) {
            const u32 m = (lo + hi) >> 1;
            if (lc[t9_w16_phys(ab + m)] <= lc[t9_w16_phys(bb + d - m - 1)])
                lo = m + 1;
            else hi = m;
        }
        /* both run heads live in registers; each step emits the
         * smaller one and reads only that side's successor. An
         * exhausted run reads as ~0, above every live composite
         * (60 bits) and equal to the pads, which never leave. */
        u32 ia = ab + lo, ib = bb + (d - lo);
        const u32 ea = bb, eb = bb + L;
        /* reads are unconditional at a clamped index and the value is
         * selected afterwards: no divergent branch per step */
        const u64 a0 = lc[t9_w16_phys(ia < ea ? ia : ab)];
        const u64 b0 = lc[t9_w16_phys(ib < eb ? ib : ab)];
        u64 a = (ia < ea) ? a0 : ~0ull;
        u64 b = (ib < eb) ? b0 : ~0ull;
#pragma unroll
        for (int r = 0; r < E; ++r) {
            const bool ta = a <= b;
            c[r] = ta ? a : b;
            if (r + 1 < E) {
                ia += ta ? 1u : 0u;
                ib += ta ? 0u : 1u;
                const u32 nx = ta ? ia : ib;
                const bool in = nx < (ta ? ea : eb);
                const u64 ld = lc[t9_w16_phys(in ? nx : ab)];
                const u64 nv = in ? ld : ~0ull;
                a = ta ? nv : a;
                b = ta ? b : nv;
            }
        }
    }

    /* the sorted composites go back into lc so that the write-back is
     * contiguous: lane t handles output positions p = t + BLOCK * r */
    __syncthreads();
    t9_w16_row_store(lc, lane, c);
    __syncthreads();
    if (REC) {
        /* ties among my 16 sorted elements and against the next lane's
         * first; a pad (~0) equals no live element, and pad pairs are
         * excluded by the bound */
        const u64 nxt = (e0 + E < (u32)NSORT) ? lc[t9_w16_phys(e0 + E)]
                                              : ~0ull;
        u32 cnt = 0;
#pragma unroll
        for (int r = 0; r < E; ++r) {
            const u64 hi = (r + 1 < E) ? c[r + 1] : nxt;
            cnt += (e0 + r + 1 < ns) && ((c[r] >> 12) == (hi >> 12));
        }
        if (cnt) atomicAdd(&s_ntie, cnt);
    }
    /* values re-gathered from the embedded original positions. All reads
     * complete before any lane writes (barrier), since the sort is in
     * place. */
    u32 v[HAS_VAL ? E : 1];
    if (HAS_VAL) {
#pragma unroll
        for (int r = 0; r < E; ++r) {
            const u32 p = lane + (u32)BLOCK * r;
            if (p < ns) v[r] = vb[(u32)lc[t9_w16_phys(p)] & 0xFFFu];
        }
    }
    __syncthreads();
    const u32 nt = REC ? s_ntie : 0u;
    if (REC && lane == 0 && nt) atomicAdd(ntied, nt);
    if (HAS_VAL) {
#pragma unroll
        for (int r = 0; r < E; ++r) {
            const u32 p = lane + (u32)BLOCK * r;
            if (p < ns) vb[p] = v[r];
        }
    }
    /* lc still holds the sorted composites (nothing wrote it since) */
    if (!REC || nt) {
#pragma unroll
        for (int r = 0; r < E; ++r) {
            const u32 p = lane + (u32)BLOCK * r;
            if (p < ns) kb[p] = high16 | (lc[t9_w16_phys(p)] >> 12);
        }
    }
}

/* ------------------------------------------------------------------ *
 * k_wave16_sort_gather: the record sort's sub-bucket sort and payload
 * gather in one kernel (1024 tier, 100-byte records). The block runs the
 * k_wave16_sort_sub<1024, 64, true, true> body on its sub-bucket and then
 * copies that sub-bucket's records, out[gbase + i] = rin[idx[i]], so the
 * sort's latency chain sits inside the gather's slot-time instead of
 * ahead of it and the sorted index is never read back from memory.
 *
 * Phases and who owns lc:
 *   1 load, blocksort, tie count    lc = composites (as the plain kernel)
 *   2 short ties settled (TIES)     lc = composites, position fields of
 *                                   equal-key runs of <= T9_FUSED_RUNMAX
 *                                   swapped into full-record order
 *   3 values and keys written back  lc = composites (read only)
 *   4 gather                        lc = the ns sorted record indices, u32
 * Tie protocol (invariants of k_wave16_sort_sub kept): d_idx is always
 * written; the keys of a sub-bucket with ANY equal neighbours are written,
 * settled or not, so a later k_tie_flags never meets equal keys in an
 * unsorted sub-bucket. Only the ties the block could not settle go to
 * *ntied (runs longer than T9_FUSED_RUNMAX, the all-equal shortcut); such
 * a block skips its gather, and every block skips it once *ntied is
 * non-zero, as the output is then redone by the tie path and the full
 * gather. *ntied == 0 after the kernel therefore means: out is complete.
 * ------------------------------------------------------------------ */
#define T9_FUSED_RUNMAX 8

/* strict bytewise less on bytes 8..99 of two 100-byte records */
__device__ __forceinline__ bool t9_rec100_tail_less(
    const u32* __restrict__ rin, u32 ra, u32 rb) {
    const u32* a = rin + (u64)ra * 25;
    const u32* b = rin + (u64)rb * 25;
#pragma unroll 1
    for (int w = 2; w < 25; ++w) {
        const u32 x = __builtin_bswap32(a[w]), y = __builtin_bswap32(b[w]);
        if (x != y) return x < y;
    }
    return false;
}

template <int D, bool TIES>
__global__ __launch_bounds__(64, 2) void k_wave16_sort_gather(
    u64* __restrict__ keys, u32* __restrict__ vals,
    const u32* __restrict__ sub_start, const u32* __restrict__ sub_n,
    u32* ntied, const u32* __restrict__ rin, u32* __restrict__ rout) {
    constexpr int NSORT = 1024, BLOCK = 64, E = 16, ROUNDS = 6, RW = 25;
    __shared__ __attribute__((aligned(16))) u64 lc[NSORT];
    __shared__ u32 s_differ;
    __shared__ u32 s_ntie;
    __shared__ u32 s_settled;

    const u32 sb = blockIdx.x;
    const u32 ns = sub_n[sb];
    if (ns == 0 || ns > (u32)NSORT) return;
    const u32 gbase = sub_start[sb];
    const u32 lane = threadIdx.x;
    const u32 e0 = lane * E;
    u32* const ob = rout + (u64)gbase * RW;

    if (ns == 1) {
        /* nothing to sort; the single record still has to be copied */
        if (__hip_atomic_load(ntied, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT))
            return;
        if (lane < (u32)RW) ob[lane] = rin[(u64)vals[gbase] * RW + lane];
        return;
    }

    if (lane == 0) { s_differ = 0; s_ntie = 0; s_settled = 0; }
    __syncthreads();

    const u64 mask48 = 0x0000FFFFFFFFFFFFull;
    const u64 high16 = keys[gbase] & ~mask48;
    const u64 ref48 = keys[gbase] & mask48;

    u64 c[E];
    u32 differ = 0;
    u64* const kb = keys + gbase;
    u32* const vb = vals + gbase;
#pragma unroll
    for (int r = 0; r < E; ++r) {
        const u32 p = lane + (u32)BLOCK * r;
        u64 cc = ~0ull;
        if (p < ns) {
            const u64 k = kb[p];
            cc = ((k & mask48) << 12) | (u64)p;
            differ |= ((k & mask48) != ref48);
        }
        lc[t9_w16_phys(p)] = cc;
    }
    if (differ) s_differ = 1;
    __syncthreads();
    if (!s_differ) {
        /* all keys equal: ns - 1 ties for the tie path, no gather */
        if (lane == 0) atomicAdd(ntied, ns - 1);
        return;
    }
    t9_w16_row_load(lc, lane, c);

    t9_w16_blocksort<E, ROUNDS>(lc, lane, c);

    __syncthreads();
    t9_w16_row_store(lc, lane, c);
    __syncthreads();
    {
        const u64 nxt = (e0 + E < (u32)NSORT) ? lc[t9_w16_phys(e0 + E)]
                                              : ~0ull;
        u32 cnt = 0;
#pragma unroll
        for (int r = 0; r < E; ++r) {
            const u64 hi = (r + 1 < E) ? c[r + 1] : nxt;
            cnt += (e0 + r + 1 < ns) && ((c[r] >> 12) == (hi >> 12));
        }
        if (cnt) atomicAdd(&s_ntie, cnt);
    }
    __syncthreads();
    const u32 nt = s_ntie;   /* equal neighbours, settled or not */
    if (TIES && nt) {
        /* each lane settles the runs that START among its 16 elements: a
         * run of <= T9_FUSED_RUNMAX equal keys is insertion-sorted by the
         * rest of the record (strict less, so true duplicates keep input
         * order) by swapping the 12-bit position fields only. Runs are
         * disjoint, and other lanes' swaps never touch the key bits that
         * the scans below compare. vb still holds the unsorted indices. */
        u32 settled = 0;
#pragma unroll 1
        for (u32 e = e0; e < e0 + E && e + 1 < ns; ++e) {
            const u64 key = lc[t9_w16_phys(e)] >> 12;
            if ((lc[t9_w16_phys(e + 1)] >> 12) != key) continue;
            if (e > 0 && (lc[t9_w16_phys(e - 1)] >> 12) == key) continue;
            u32 len = 2;
            while (len <= T9_FUSED_RUNMAX && e + len < ns &&
                   (lc[t9_w16_phys(e + len)] >> 12) == key)
                ++len;
            if (len > T9_FUSED_RUNMAX) continue;   /* left to the tie path */
            for (u32 i = 1; i < len; ++i)
                for (u32 j = i; j > 0; --j) {
                    const u32 hi_at = t9_w16_phys(e + j);
                    const u32 lo_at = t9_w16_phys(e + j - 1);
                    const u64 ch = lc[hi_at], cl = lc[lo_at];
                    const u32 ph = (u32)ch & 0xFFFu, pl = (u32)cl & 0xFFFu;
                    if (!t9_rec100_tail_less(rin, vb[ph], vb[pl])) break;
                    lc[hi_at] = (ch & ~0xFFFull) | pl;
                    lc[lo_at] = (cl & ~0xFFFull) | ph;
                }
            settled += len - 1;
        }
        if (settled) atomicAdd(&s_settled, settled);
    }
    __syncthreads();
    /* the sorted record indices, re-gathered from the embedded original
     * positions; all reads complete before any lane writes (barrier) */
    u32 v[E];
#pragma unroll
    for (int r = 0; r < E; ++r) {
        const u32 p = lane + (u32)BLOCK * r;
        if (p < ns) v[r] = vb[(u32)lc[t9_w16_phys(p)] & 0xFFFu];
    }
    __syncthreads();
    const u32 unsettled = nt - s_settled;
    if (lane == 0 && unsettled) atomicAdd(ntied, unsettled);
#pragma unroll
    for (int r = 0; r < E; ++r) {
        const u32 p = lane + (u32)BLOCK * r;
        if (p < ns) vb[p] = v[r];
    }
    if (nt) {
#pragma unroll
        for (int r = 0; r < E; ++r) {
            const u32 p = lane + (u32)BLOCK * r;
            if (p < ns) kb[p] = high16 | (lc[t9_w16_phys(p)] >> 12);
        }
    }
    if (unsettled) return;   /* the tie path redoes the output */

    /* ---- gather phase: lc becomes the index buffer ---- */
    __syncthreads();
    u32* const li = (u32*)lc;
#pragma unroll
    for (int r = 0; r < E; ++r) {
        const u32 p = lane + (u32)BLOCK * r;
        if (p < ns) li[p] = v[r];
    }
    __syncthreads();
    if (__hip_atomic_load(ntied, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        return;
    /* word-wise, consecutive lanes on consecutive output words (the
     * access shape of k_gather_records_span), D independent loads in
     * flight per lane */
    const u32 W = ns * RW;
    for (u32 g0 = lane; g0 < W; g0 += (u32)BLOCK * D) {
        u32 x[D];
        if (g0 - lane + (u32)BLOCK * D <= W) {
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const u32 g = g0 + (u32)BLOCK * j;
                const u32 rec = g / (u32)RW;
                x[j] = rin[(u64)li[rec] * RW + (g - rec * RW)];
            }
#pragma unroll
            for (int j = 0; j < D; ++j) ob[g0 + (u32)BLOCK * j] = x[j];
        }
        else {
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const u32 g = g0 + (u32)BLOCK * j;
                if (g < W) {
                    const u32 rec = g / (u32)RW;
                    x[j] = rin[(u64)li[rec] * RW + (g - rec * RW)];
                }
            }
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const u32 g = g0 + (u32)BLOCK * j;
                if (g < W) ob[g] = x[j];
            }
        }
    }
}

/* ------------------------------------------------------------------ *
 * k_wave16_sort_gather_packed: the same kernel over the packed pass-2
 * output (k_scatter_seg9_packed): one u64 composite per element,
 * C = (key bits 46..10) << T9_PK_IBITS | record index. C is already a
 * stable sort key, so the block sorts the ns composites as they are: no
 * position field, no index array to re-gather from, and nothing is written
 * back but the records.
 *
 * The composite drops key bits 9..0, so neighbours with equal C >> IBITS
 * are only CANDIDATE ties: true ones (equal 8-byte keys, to be ordered by
 * bytes 8..99) or false ones (keys that differ in the dropped bits). Both
 * are settled the same way: a candidate run of <= T9_FUSED_RUNMAX is
 * insertion-sorted by the full order, the record's 64-bit key (big-endian,
 * or native under keyle) and then its bytes 8..99, by swapping the index
 * fields. The less is strict and a run starts in index order, so true
 * duplicates keep input order. What the block cannot settle (a longer run)
 * goes to *ntied and the block skips its gather; every block skips it once
 * *ntied is non-zero. *ntied == 0 after the kernel means: out is complete.
 * Otherwise the caller reruns pass 2 and the sort in the wide form.
 * A pad is ~0; a live composite can equal it only at index 2^27 - 1 with
 * all kept key bits set, and then the two are the same value wherever the
 * merge puts them.
 * ------------------------------------------------------------------ */
__device__ __forceinline__ bool t9_rec100_less(
    const u32* __restrict__ rin, u32 ra, u32 rb, bool keyle) {
    const u32* a = rin + (u64)ra * 25;
    const u32* b = rin + (u64)rb * 25;
    const u32 a0 = a[0], a1 = a[1], b0 = b[0], b1 = b[1];
    const u64 ka = keyle ? (((u64)a1 << 32) | a0)
                         : (((u64)__builtin_bswap32(a0) << 32) |
                            __builtin_bswap32(a1));
    const u64 kb = keyle ? (((u64)b1 << 32) | b0)
                         : (((u64)__builtin_bswap32(b0) << 32) |
                            __builtin_bswap32(b1));
    if (ka != kb) return ka < kb;
    return t9_rec100_tail_less(rin, ra, rb);
}

/* record index of a composite. It is below n by construction; the clamp to
 * imax = n - 1 keeps a damaged workspace from becoming a wild read. */
__device__ __forceinline__ u32 t9_pk_idx(u64 c, u32 imax) {
    const u32 i = (u32)c & T9_PK_IMASK;
    return i < imax ? i : imax;
}

template <int D>
__global__ __launch_bounds__(64, 2) void k_wave16_sort_gather_packed(
    const u64* __restrict__ comp, const u32* __restrict__ sub_start,
    const u32* __restrict__ sub_n, u32* ntied, const u32* __restrict__ rin,
    u32* __restrict__ rout, u32 keyle, u32 imax) {
    constexpr int NSORT = 1024, BLOCK = 64, E = 16, ROUNDS = 6, RW = 25;
    constexpr int IB = T9_PK_IBITS;
    __shared__ __attribute__((aligned(16))) u64 lc[NSORT];
    __shared__ u32 s_ntie;
    __shared__ u32 s_settled;

    const u32 sb = blockIdx.x;
    const u32 ns = sub_n[sb];
    if (ns == 0 || ns > (u32)NSORT) return;
    const u32 gbase = sub_start[sb];
    const u32 lane = threadIdx.x;
    const u32 e0 = lane * E;
    u32* const ob = rout + (u64)gbase * RW;
    const u64* const cb = comp + gbase;

    if (ns == 1) {
        if (__hip_atomic_load(ntied, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT))
            return;
        const u32 idx = t9_pk_idx(cb[0], imax);
        if (lane < (u32)RW) ob[lane] = rin[(u64)idx * RW + lane];
        return;
    }

    if (lane == 0) { s_ntie = 0; s_settled = 0; }

    u64 c[E];
#pragma unroll
    for (int r = 0; r < E; ++r) {
        const u32 p = lane + (u32)BLOCK * r;
        /* unconditional at a clamped position, so that the 16 loads are
         * in flight together and not one per branch */
        const u64 cc = cb[p < ns ? p : ns - 1];
        lc[t9_w16_phys(p)] = (p < ns) ? cc : ~0ull;
    }
    __syncthreads();
    t9_w16_row_load(lc, lane, c);

    t9_w16_blocksort<E, ROUNDS>(lc, lane, c);

    __syncthreads();
    t9_w16_row_store(lc, lane, c);
    __syncthreads();
    {
        const u64 nxt = (e0 + E < (u32)NSORT) ? lc[t9_w16_phys(e0 + E)]
                                              : ~0ull;
        u32 cnt = 0;
#pragma unroll
        for (int r = 0; r < E; ++r) {
            const u64 hi = (r + 1 < E) ? c[r + 1] : nxt;
            cnt += (e0 + r + 1 < ns) && ((c[r] >> IB) == (hi >> IB));
        }
        if (cnt) atomicAdd(&s_ntie, cnt);
    }
    __syncthreads();
    const u32 nt = s_ntie;   /* candidate neighbours, settled or not */
    if (nt) {
        /* each lane settles the runs that START among its 16 elements;
         * runs are disjoint, and the swaps leave the key bits that the
         * scans compare alone */
        u32 settled = 0;
#pragma unroll 1
        for (u32 e = e0; e < e0 + E && e + 1 < ns; ++e) {
            const u64 key = lc[t9_w16_phys(e)] >> IB;
            if ((lc[t9_w16_phys(e + 1)] >> IB) != key) continue;
            if (e > 0 && (lc[t9_w16_phys(e - 1)] >> IB) == key) continue;
            u32 len = 2;
            while (len <= T9_FUSED_RUNMAX && e + len < ns &&
                   (lc[t9_w16_phys(e + len)] >> IB) == key)
                ++len;
            if (len > T9_FUSED_RUNMAX) continue;   /* left to the wide redo */
            for (u32 i = 1; i < len; ++i)
                for (u32 j = i; j > 0; --j) {
                    const u32 hi_at = t9_w16_phys(e + j);
                    const u32 lo_at = t9_w16_phys(e + j - 1);
                    const u64 ch = lc[hi_at], cl = lc[lo_at];
                    const u32 ih = (u32)ch & T9_PK_IMASK;   /* swapped as is */
                    const u32 il = (u32)cl & T9_PK_IMASK;
                    if (!t9_rec100_less(rin, ih < imax ? ih : imax,
                                        il < imax ? il : imax, keyle != 0))
                        break;
                    lc[hi_at] = (ch & ~(u64)T9_PK_IMASK) | il;
                    lc[lo_at] = (cl & ~(u64)T9_PK_IMASK) | ih;
                }
            settled += len - 1;
        }
        if (settled) atomicAdd(&s_settled, settled);
    }
    __syncthreads();
    /* the sorted record indices */
    u32 v[E];
#pragma unroll
    for (int r = 0; r < E; ++r) {
        const u32 p = lane + (u32)BLOCK * r;
        v[r] = t9_pk_idx(lc[t9_w16_phys(p)], imax);
    }
    const u32 unsettled = nt - s_settled;
    if (lane == 0 && unsettled) atomicAdd(ntied, unsettled);
    if (unsettled) return;   /* the wide redo produces the output */

    /* ---- gather phase: lc becomes the index buffer ---- */
    __syncthreads();
    u32* const li = (u32*)lc;
#pragma unroll
    for (int r = 0; r < E; ++r) {
        const u32 p = lane + (u32)BLOCK * r;
        if (p < ns) li[p] = v[r];
    }
    __syncthreads();
    if (__hip_atomic_load(ntied, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        return;
    /* the word loop of k_wave16_sort_gather. The word index is made
     * opaque once per trip: left to itself the compiler widens it to 64
     * bits and carries the 16 divisions by 25 across the loop in 64-bit
     * registers (130 VGPRs against 76). */
    const u32 W = ns * RW;
    for (u32 gb = 0; gb < W; gb += (u32)BLOCK * D) {
        u32 g0 = gb + lane;
        asm volatile("" : "+v"(g0));
        u32 x[D];
        if (gb + (u32)BLOCK * D <= W) {
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const u32 g = g0 + (u32)BLOCK * j;
                const u32 rec = g / (u32)RW;
                x[j] = rin[(u64)li[rec] * RW + (g - rec * RW)];
            }
#pragma unroll
            for (int j = 0; j < D; ++j) ob[g0 + (u32)BLOCK * j] = x[j];
        }
        else {
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const u32 g = g0 + (u32)BLOCK * j;
                if (g < W) {
                    const u32 rec = g / (u32)RW;
                    x[j] = rin[(u64)li[rec] * RW + (g - rec * RW)];
                }
            }
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const u32 g = g0 + (u32)BLOCK * j;
                if (g < W) ob[g] = x[j];
            }
        }
    }
}

/* wave16 span sort (3-level path, PASSES=6 spans): same blocksort as
 * k_wave16_sort_sub, but out-of-place over span descriptors. Valid for
 * the 6-pass span case only: spans pack (b7,b6,b5) groups that share
 * their top 16 key bits, so the 60-bit stable composite applies.
 * Oversize spans copy through (the ranged-LSD fallback re-sorts them),
 * mirroring k_lds_sort_span. in == out is safe: a block barrier
 * separates every global read from the first global write. */
template <int NSORT, int BLOCK, bool HAS_VAL>
__global__ __launch_bounds__(BLOCK, 2) void k_wave16_sort_span(
    const u64* __restrict__ keys_in, const u32* __restrict__ vals_in,
    u64* __restrict__ keys_out, u32* __restrict__ vals_out,
    const u32* __restrict__ span_start, const u32* __restrict__ span_len) {
    constexpr int E = NSORT / BLOCK;
    static_assert(E == 16, "wave16 mapping: 16 elements per lane");
    constexpr int ROUNDS = (NSORT == 1024) ? 6 : (NSORT == 2048) ? 7 : 8;
    __shared__ u64 lc[NSORT];
    __shared__ u32 s_differ;

    const u32 sb = blockIdx.x;
    const u32 ns = span_len[sb];
    if (ns == 0) return;
    const u32 gbase = span_start[sb];
    const u32 lane = threadIdx.x;
    const u32 e0 = lane * E;

    if (ns > (u32)NSORT) {
        if (keys_out != keys_in)
            for (u32 i = lane; i < ns; i += BLOCK) {
                keys_out[gbase + i] = keys_in[gbase + i];
                if (HAS_VAL) vals_out[gbase + i] = vals_in[gbase + i];
            }
        return;
    }

    if (lane == 0) s_differ = 0;
    __syncthreads();

    const u64 mask48 = 0x0000FFFFFFFFFFFFull;
    const u64 high16 = keys_in[gbase] & ~mask48;
    const u64 ref48 = keys_in[gbase] & mask48;

    /* values never travel through the sort (positions embedded in the
     * composite; re-gathered at writeback — see k_wave16_sort_sub) */
    u64 c[E];
    u32 differ = 0;
#pragma unroll
    for (int r = 0; r < E; ++r) {
        const u32 i = e0 + r;
        if (i < ns) {
            const u64 k = keys_in[gbase + i];
            c[r] = ((k & mask48) << 12) | (u64)i;
            differ |= ((k & mask48) != ref48);
        } else {
            c[r] = ~0ull;
        }
    }
    if (differ) s_differ = 1;
    __syncthreads();
    if (!s_differ) {
        if (keys_out != keys_in) {
#pragma unroll
            for (int r = 0; r < E; ++r) {
                const u32 i = e0 + r;
                if (i < ns) {
                    keys_out[gbase + i] = high16 | ((c[r] >> 12) & mask48);
                    if (HAS_VAL) vals_out[gbase + i] = vals_in[gbase + i];
                }
            }
        }
        return;
    }

#pragma unroll
    for (int lk = 1; lk <= 4; ++lk) {
        const int k = 1 << lk;
#pragma unroll
        for (int lj = lk - 1; lj >= 0; --lj) {
            const int j = 1 << lj;
#pragma unroll
            for (int r = 0; r < E; ++r) {
                const int q = r ^ j;
                if (q > r) {
                    const bool asc = (r & k) == 0;
                    if ((c[r] > c[q]) == asc) {
                        u64 tc = c[r]; c[r] = c[q]; c[q] = tc;
                    }
                }
            }
        }
    }

#pragma unroll
    for (int lm = 0; lm < ROUNDS; ++lm) {
        const u32 L = (u32)E << lm;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < E; ++r) lc[e0 + r] = c[r];
        __syncthreads();
        const u32 pairbase = e0 & ~(2 * L - 1);
        const u32 d = e0 - pairbase;
        const u64* A = lc + pairbase;
        const u64* B = lc + pairbase + L;
        u32 lo = (d > L) ? d - L : 0;
        u32 hi = (d < L) ? d : L;
        while (lo < hi) {
            const u32 m = (lo + hi) >> 1;
            if (A[m] <= B[d - m - 1]) lo = m + 1;
            else hi = m;
        }
        u32 i = lo, j = d - lo;
#pragma unroll
        for (int r = 0; r < E; ++r) {
            const bool ta = (j >= L) || (i < L && A[i] <= B[j]);
            c[r] = (ta ? A[i] : B[j]);
            if (ta) ++i; else ++j;
        }
    }

    /* gather values from their embedded original positions, then write
     * (barrier keeps all reads ahead of the in-place writes) */
    u32 v[HAS_VAL ? E : 1];
    if (HAS_VAL) {
#pragma unroll
        for (int r = 0; r < E; ++r) {
            const u32 i = e0 + r;
            if (i < ns) v[r] = vals_in[gbase + (u32)(c[r] & 0xFFFu)];
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < E; ++r) {
        const u32 i = e0 + r;
        if (i < ns) {
            keys_out[gbase + i] = high16 | (c[r] >> 12);
            if (HAS_VAL) vals_out[gbase + i] = v[r];
        }
    }
}
