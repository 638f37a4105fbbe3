/* t9_sort_msb9.hip — 9-bit level-2 digit for the two-level MSB pipeline.
 * This is the PRODUCTION DEFAULT for 2^22 <= n < T9_L3_MIN
 * (pass2_bits() in t9_sort_msb.hip defaults to 9; T9_PASS2_BITS=8 is the
 * byte-digit fallback): 256 x 512 = 131072
 * (b7, 9-bit) sub-buckets of ~n/131072 elements, so the level-3 LDS sort
 * runs the 1024-element / 256-thread variant at ~5 blocks per CU — the
 * measured limiter of the 8-bit flow was the LDS sort's barrier parking
 * at 2 blocks per CU. Level-2 digit = key bits 47..55; level 3 sorts the
 * low 47 bits (6 passes, bit 47 re-covered harmlessly).
 *
 * Self-contained variants of hist/seg-scan/scatter over 512 digits with
 * u16 count rows; digit-of-slot is recomputed from the staged key
 * instead of stored. Shares the pass-1 machinery and fallbacks with
 * t9_sort_msb.hip via its exported helpers.
 *
 * k_scatter_seg9_packed is the scatter of the packed record sort (n <= 2^27,
 * fused sort + gather): one u64 composite per element instead of the
 * (u64 key, u32 index) pair, one trip through the reorder buffer.
 */

#include "t9_common.h"
#include "t9_rank_scatter.h"

#include <cstdlib>
#include <vector>

#define T9_MSB_TILE 8192
#define NDIG9 512

__device__ inline u32 bucket_of9(const u32* s_abase, u32 pos) {
    u32 lo = 0, hi = 255;
    while (lo < hi) {
        u32 mid = (lo + hi + 1) >> 1;
        if (s_abase[mid] <= pos) lo = mid; else hi = mid - 1;
    }
    return lo;
}

/* segmented per-block histogram over the padded pass-1 output, 512 bins */
__global__ __launch_bounds__(256) void k_hist_seg9(
    const u64* __restrict__ keys, const u32* __restrict__ abase,
    const u32* __restrict__ bucket_n, u32* __restrict__ hist) {
    __shared__ u32 s_cnt[NDIG9];
    __shared__ u32 s_abase[257];
    const u32 tid = threadIdx.x;
    s_abase[tid] = abase[tid];
    if (tid == 0) s_abase[256] = abase[256];
    s_cnt[tid] = 0;
    s_cnt[tid + 256] = 0;
    __syncthreads();
    /* u64 tile base before narrowing (grid is B2max-sized; see the same
     * guard in t9_sort_msb.hip k_hist_seg — ADVICE r01, medium) */
    const u64 tbase64 = (u64)blockIdx.x * T9_MSB_TILE;
    if (tbase64 < s_abase[256]) {
        const u32 tbase = (u32)tbase64;
        const u32 b = bucket_of9(s_abase, tbase);
        const u32 off = tbase - s_abase[b];
        const u32 tn = (bucket_n[b] > off)
                           ? ((bucket_n[b] - off < T9_MSB_TILE)
                                  ? bucket_n[b] - off
                                  : T9_MSB_TILE)
                           : 0;
        const u32 lane = tid & 63;
        for (u32 i0 = 0; i0 < (u32)T9_MSB_TILE; i0 += 256) {
            const u32 i = i0 + tid;
            const bool valid = i < tn;
            const u32 d =
                valid ? (u32)(keys[tbase + i] >> 47) & 511u : 0;
            t9_hist_ballot_add<9>(s_cnt, d, valid, lane);
        }
    }
    __syncthreads();
    hist[(u64)blockIdx.x * NDIG9 + tid] = s_cnt[tid];
    hist[(u64)blockIdx.x * NDIG9 + tid + 256] = s_cnt[tid + 256];
}

/* per-bucket segmented column scan over 512 digits (thread t owns digits
 * t and t+256) -> final offsets in hist, sub index arrays */
__global__ __launch_bounds__(256) void k_seg_scan9(
    u32* __restrict__ hist, const u32* __restrict__ abase,
    const u32* __restrict__ bucket_n, const u32* __restrict__ true_base,
    u32* __restrict__ sub_start, u32* __restrict__ sub_n) {
    const u32 b = blockIdx.x;
    const u32 tid = threadIdx.x;
    const u32 r0 = abase[b] / T9_MSB_TILE;
    const u32 rows = (bucket_n[b] + T9_MSB_TILE - 1) / T9_MSB_TILE;
    u32 tot0 = 0, tot1 = 0;
    for (u32 r = 0; r < rows; ++r) {
        tot0 += hist[(u64)(r0 + r) * NDIG9 + tid];
        tot1 += hist[(u64)(r0 + r) * NDIG9 + tid + 256];
    }
    __shared__ u32 sh[NDIG9];
    sh[tid] = tot0;
    sh[tid + 256] = tot1;
    __syncthreads();
    t9_scan_onewave<NDIG9>(sh, tid);
    __syncthreads();
    const u32 gstart0 = true_base[b] + sh[tid];
    const u32 gstart1 = true_base[b] + sh[tid + 256];
    sub_start[(u64)b * NDIG9 + tid] = gstart0;
    sub_start[(u64)b * NDIG9 + tid + 256] = gstart1;
    sub_n[(u64)b * NDIG9 + tid] = tot0;
    sub_n[(u64)b * NDIG9 + tid + 256] = tot1;
    u32 run0 = gstart0, run1 = gstart1;
    for (u32 r = 0; r < rows; ++r) {
        u32 v0 = hist[(u64)(r0 + r) * NDIG9 + tid];
        u32 v1 = hist[(u64)(r0 + r) * NDIG9 + tid + 256];
        hist[(u64)(r0 + r) * NDIG9 + tid] = run0;
        hist[(u64)(r0 + r) * NDIG9 + tid + 256] = run1;
        run0 += v0;
        run1 += v1;
    }
}

/* Segmented 1024-thread stable scatter over 512 digits, one 8192-key tile
 * of the padded pass-1 output per block.
 *
 * LDS bounds the residency: the block holds exactly 80 KiB (the 64 KiB
 * reorder buffer and the 16 KiB count array, nothing else), so two blocks
 * (8 waves/SIMD) share a CU's 160 KiB and one runs while the other waits
 * on its loads or drains its stores. To fit, each lane keeps its 8 keys,
 * their ranks, tile positions and output positions in registers (every key
 * is read from global memory once); one u16 array holds the per-wave
 * counts and then, in place, the tile position at which each wave's run of
 * each digit starts; the keys and then the values are reordered through
 * the same buffer; the tile's bucket is found from abase in global memory
 * (no LDS copy); and the two small arrays that are left overlay bytes that
 * are dead while they live:
 *
 *   s_raw    keys from barrier C (round 1 writes them) to barrier F (every
 *            thread holds its 8 reordered keys in registers), values from
 *            barrier F on;
 *   s_wtot   s_raw[0, 32): written between barriers A and B, read between
 *            B and C, before the first key is written to s_raw;
 *   s_wcnt   counts and tile positions up to barrier D, after which no
 *            count is read again;
 *   s_delta  s_wcnt[0, 2048): written between barriers D and E, read
 *            between E and F.
 */
template <bool HAS_VAL>
__global__ __launch_bounds__(1024, 8) void k_scatter_seg9(
    const u64* __restrict__ in_keys, const u32* __restrict__ in_vals,
    const u32* __restrict__ abase, const u32* __restrict__ bucket_n,
    u64* __restrict__ out_keys, u32* __restrict__ out_vals,
    const u32* __restrict__ offs) {
    constexpr int TILE = T9_MSB_TILE;
    constexpr int NW = 16;
    constexpr int SUB = TILE / NW;
    constexpr int GROUPS = SUB / 64;   /* = TILE / 1024: keys per lane */
    /* keys in round 1, values in round 2 */
    __shared__ __align__(16) u8 s_raw[TILE * 8];
    u64* const s_okeys = (u64*)s_raw;
    u32* const s_ovals = (u32*)s_raw;
    /* per wave and digit: first the count (<= SUB = 512, a wave's
     * sub-tile), then the tile position of the wave's first key of that
     * digit (<= 8191 where a key uses it, TILE where none does) */
    static_assert(SUB <= 65535 && TILE <= 65535, "u16 counts and offsets");
    static_assert(NW * 64 == 1024 && NDIG9 == 8 * 64,
                  "one thread per key column, waves 0..7 own the digits");
    __shared__ __align__(16) u16 s_wcnt[NW * NDIG9];
    /* totals of the digits of waves 0..7, for the scan across them */
    u32* const s_wtot = (u32*)s_raw;
    /* per digit: output position of the digit's run minus its tile
     * position; u32 arithmetic, the sum with a tile position is exact */
    u32* const s_delta = (u32*)s_wcnt;

    const u32 tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    /* Which tile: blocks are dealt to the 8 XCDs in turn, so block b and
     * b + 8 share an L2. Each XCD takes a contiguous eighth of the tiles:
     * the tiles in flight on it are neighbours, mostly of one bucket, and
     * the short digit runs (16 keys on average) that they append to the
     * same sub-buckets meet in that L2 before they leave it. Any bijection
     * is correct; this one is for speed only. */
    const u32 xper = gridDim.x >> 3, xrem = gridDim.x & 7;
    const u32 xcd = blockIdx.x & 7;
    const u32 tile = xcd * xper + (xcd < xrem ? xcd : xrem) +
                     (blockIdx.x >> 3);
    /* u64 guard before narrowing — see k_hist_seg9 */
    const u64 tbase64 = (u64)tile * TILE;
    if (tbase64 >= abase[256]) return;
    const u32 tbase = (u32)tbase64;

    /* One round of loads, all in flight together: the lane's 8 keys, and
     * abase and bucket_n, 4 entries a lane in every wave. The keys do not
     * wait for the tile's length: a tile below abase[256] lies inside the
     * padded pass-1 output whole, and what it holds past its length is
     * read and never used. */
    const u32 wbase = wave * SUB;
    u64 key[GROUPS];
#pragma unroll
    for (int g = 0; g < GROUPS; ++g)
        key[g] = in_keys[tbase + wbase + g * 64 + lane];
    u32 ab[4], bnq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        ab[q] = abase[q * 64 + lane];
        bnq[q] = bucket_n[q * 64 + lane];
    }
    u16* const wc = s_wcnt + wave * NDIG9;
    for (u32 t = lane; t < NDIG9; t += 64) wc[t] = 0;

    /* bucket of the tile: abase is non-decreasing with abase[0] = 0, so the
     * last b with abase[b] <= tbase is the count of such entries less one
     * (what bucket_of9 finds); no LDS copy, no barrier. Its base and count
     * come from the lane that loaded them. */
    u32 nle = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        nle += (u32)__popcll(__ballot(ab[q] <= tbase));
    const u32 b = nle - 1, bq = b >> 6;
    const u32 ab_b = (u32)__builtin_amdgcn_readlane(
        (int)(bq == 0 ? ab[0] : bq == 1 ? ab[1] : bq == 2 ? ab[2] : ab[3]),
        (int)(b & 63));
    const u32 bn = (u32)__builtin_amdgcn_readlane(
        (int)(bq == 0 ? bnq[0] : bq == 1 ? bnq[1] : bq == 2 ? bnq[2]
                                                            : bnq[3]),
        (int)(b & 63));
    const u32 off_in_bucket = tbase - ab_b;
    const u32 tn = (bn > off_in_bucket)
                       ? ((bn - off_in_bucket < (u32)TILE)
                              ? bn - off_in_bucket
                              : (u32)TILE)
                       : 0;
    if (tn == 0) return;   /* padding of an empty bucket tail: block-uniform */

    /* rank inside the wave's sub-tile, then position inside the tile.
     * differ = the lanes whose digit is not this lane's: bit by bit, the
     * ballot of the bit, inverted for a lane whose own bit is set.
     * Ranks (< 512) and tile positions (< 8192) are kept two to a
     * register, in 16 bits each. */
    u32 pos2[GROUPS / 2] = {};
#pragma unroll
    for (int g = 0; g < GROUPS; ++g) {
        const u32 i = wbase + g * 64 + lane;
        const bool valid = i < tn;
        const u32 d = (u32)(key[g] >> 47) & 511u;
        u32 dlo = 0, dhi = 0;
#pragma unroll
        for (int bit = 0; bit < 9; ++bit) {
            const u32 own = 0u - ((d >> bit) & 1u);   /* all ones or zero */
            const u64 bb = __ballot(own != 0);
            dlo |= (u32)bb ^ own;
            dhi |= (u32)(bb >> 32) ^ own;
        }
        const u64 m = __ballot(valid) & ~(((u64)dhi << 32) | dlo);
        const u32 wr = (u32)__popcll(m & ((1ull << lane) - 1ull));
        const u32 before = wc[d];
        pos2[g >> 1] |= (before + wr) << (16 * (g & 1));
        if (valid && wr == 0) wc[d] = (u16)(before + (u32)__popcll(m));
    }
    u32 goff = 0;   /* used after barrier B */
    if (tid < NDIG9) goff = offs[(u64)tile * NDIG9 + tid];
    __syncthreads();                                   /* A */

    /* combine (waves 0..7, thread = digit): counts -> offsets inside the
     * digit, in place; the digit totals are scanned in registers, wave by
     * wave, and the wave totals go through s_wtot */
    u32 excl = 0;
    if (tid < NDIG9) {
        u32 run = 0;
        for (int w = 0; w < NW; ++w) {
            const u32 c = s_wcnt[w * NDIG9 + tid];
            s_wcnt[w * NDIG9 + tid] = (u16)run;
            run += c;
        }
        u32 v = run;
        for (int off = 1; off < 64; off <<= 1) {
            const u32 y = __shfl_up(v, off);
            if (lane >= (u32)off) v += y;
        }
        excl = v - run;
        if (lane == 63) s_wtot[wave] = v;
    }
    __syncthreads();                                   /* B */
    u32 delta = 0;
    if (tid < NDIG9) {
        u32 start = excl;   /* tile position of the digit's run */
        for (u32 w = 0; w < wave; ++w) start += s_wtot[w];
        for (int w = 0; w < NW; ++w)
            s_wcnt[w * NDIG9 + tid] += (u16)start;
        delta = goff - start;
    }
    __syncthreads();                                   /* C */

    /* the values, used in round 2: in flight behind round 1 and the
     * barriers up to F, and for a whole tile like the keys */
    u32 val[HAS_VAL ? GROUPS : 1];
    if constexpr (HAS_VAL) {
#pragma unroll
        for (int g = 0; g < GROUPS; ++g)
            val[g] = in_vals[tbase + wbase + g * 64 + lane];
    }

    /* round 1: keys. Here and below only the LDS writes and the global
     * stores are under a condition; the LDS reads run for a whole tile
     * (past its length they fetch what is never used), so that they go out
     * back to back and not one per branch. */
#pragma unroll
    for (int g = 0; g < GROUPS; ++g) {
        const u32 i = wbase + g * 64 + lane;
        const u32 d = (u32)(key[g] >> 47) & 511u;
        const u32 pos = ((pos2[g >> 1] >> (16 * (g & 1))) & 0xffffu) +
                        (u32)wc[d];
        if (i < tn) s_okeys[pos] = key[g];
        pos2[g >> 1] += (u32)wc[d] << (16 * (g & 1));
    }
    __syncthreads();                                   /* D */
    if (tid < NDIG9) s_delta[tid] = delta;
    __syncthreads();                                   /* E */

    /* the thread's 8 keys of the reordered tile and their output positions.
     * An output position is below the end of the output array, which the
     * u32 offsets in offs already address. */
    u64 k[GROUPS];
    u32 gpos[GROUPS];
#pragma unroll
    for (int c = 0; c < GROUPS; ++c) k[c] = s_okeys[c * 1024 + tid];
#pragma unroll
    for (int c = 0; c < GROUPS; ++c)
        gpos[c] = s_delta[(u32)(k[c] >> 47) & 511u] + (c * 1024 + tid);
    if constexpr (HAS_VAL) {
        __syncthreads();                               /* F */
        /* round 2: values, through the same buffer. They go in before the
         * key stores go out, so that the wait for the value loads is not
         * a wait for those stores as well. */
#pragma unroll
        for (int g = 0; g < GROUPS; ++g)   /* the wait, on every path */
            asm volatile("" : "+v"(val[g]));
#pragma unroll
        for (int g = 0; g < GROUPS; ++g) {
            const u32 i = wbase + g * 64 + lane;
            if (i < tn)
                s_ovals[(pos2[g >> 1] >> (16 * (g & 1))) & 0xffffu] = val[g];
        }
        __builtin_amdgcn_sched_barrier(0);   /* no store moves above */
    }
#pragma unroll
    for (int c = 0; c < GROUPS; ++c)
        if (c * 1024 + tid < tn) out_keys[gpos[c]] = k[c];
    if (!HAS_VAL) return;
    __syncthreads();                                   /* G */
    {
        u32 v[GROUPS];
#pragma unroll
        for (int c = 0; c < GROUPS; ++c) v[c] = s_ovals[c * 1024 + tid];
#pragma unroll
        for (int c = 0; c < GROUPS; ++c)
            if (c * 1024 + tid < tn) out_vals[gpos[c]] = v[c];
    }
}

/* Packed form of k_scatter_seg9 for the record sort whose sub-bucket sort
 * also gathers (k_wave16_sort_gather_packed) and n <= 2^27. After this pass
 * the top 17 key bits are implied by the sub-bucket, so one u64 per element
 * is enough: C = (key bits 46..10) << 27 | idx, itself a stable sort key
 * (the index breaks ties of the kept bits in input order). out_comp takes
 * the place of out_keys; no value array is written.
 *
 * Ranking, the tile order, the bucket search and the 80 KiB / two blocks
 * per CU are those of the wide form. The composite goes through the 64 KiB
 * buffer once; it no longer holds the digit, so the digit of each slot
 * travels next to it in bytes that are dead by then:
 *
 *   s_raw    composites from barrier C (the one reorder round) to the end;
 *   s_wtot   s_raw[0, 32): as in the wide form;
 *   s_wcnt   counts and tile positions up to barrier D;
 *   s_delta  s_wcnt bytes [0, 2048): written between D and E, read after E;
 *   s_dig8   s_wcnt bytes [2048, 10240): low 8 digit bits of every slot,
 *            written between D and E by the lane that placed the slot;
 *   s_hi     s_wcnt bytes [10240, 10244): tile position of digit 256's run.
 *            The reordered tile is sorted by digit, so slot j has digit bit
 *            8 set exactly where j >= s_hi.
 */
__global__ __launch_bounds__(1024, 8) void k_scatter_seg9_packed(
    const u64* __restrict__ in_keys, const u32* __restrict__ in_vals,
    const u32* __restrict__ abase, const u32* __restrict__ bucket_n,
    u64* __restrict__ out_comp, const u32* __restrict__ offs) {
    constexpr int TILE = T9_MSB_TILE;
    constexpr int NW = 16;
    constexpr int SUB = TILE / NW;
    constexpr int GROUPS = SUB / 64;
    __shared__ __align__(16) u8 s_raw[TILE * 8];
    u64* const s_ocomp = (u64*)s_raw;
    static_assert(SUB <= 65535 && TILE <= 65535, "u16 counts and offsets");
    static_assert(NW * 64 == 1024 && NDIG9 == 8 * 64,
                  "one thread per key column, waves 0..7 own the digits");
    __shared__ __align__(16) u16 s_wcnt[NW * NDIG9];
    u32* const s_wtot = (u32*)s_raw;
    u32* const s_delta = (u32*)s_wcnt;
    u8* const s_dig8 = (u8*)s_wcnt + NDIG9 * 4;
    u32* const s_hi = (u32*)((u8*)s_wcnt + NDIG9 * 4 + TILE);
    static_assert(NDIG9 * 4 + TILE + 4 <= NW * NDIG9 * 2,
                  "the overlays fit the count array");

    const u32 tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    /* tile order: see k_scatter_seg9 */
    const u32 xper = gridDim.x >> 3, xrem = gridDim.x & 7;
    const u32 xcd = blockIdx.x & 7;
    const u32 tile = xcd * xper + (xcd < xrem ? xcd : xrem) +
                     (blockIdx.x >> 3);
    const u64 tbase64 = (u64)tile * TILE;
    if (tbase64 >= abase[256]) return;
    const u32 tbase = (u32)tbase64;

    /* keys, indices, abase and bucket_n in one round of loads; a tile below
     * abase[256] lies inside the padded pass-1 arrays whole */
    const u32 wbase = wave * SUB;
    u64 key[GROUPS];
#pragma unroll
    for (int g = 0; g < GROUPS; ++g)
        key[g] = in_keys[tbase + wbase + g * 64 + lane];
    u32 val[GROUPS];
#pragma unroll
    for (int g = 0; g < GROUPS; ++g)
        val[g] = in_vals[tbase + wbase + g * 64 + lane];
    u32 ab[4], bnq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        ab[q] = abase[q * 64 + lane];
        bnq[q] = bucket_n[q * 64 + lane];
    }
    u16* const wc = s_wcnt + wave * NDIG9;
    for (u32 t = lane; t < NDIG9; t += 64) wc[t] = 0;

    u32 nle = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        nle += (u32)__popcll(__ballot(ab[q] <= tbase));
    const u32 b = nle - 1, bq = b >> 6;
    const u32 ab_b = (u32)__builtin_amdgcn_readlane(
        (int)(bq == 0 ? ab[0] : bq == 1 ? ab[1] : bq == 2 ? ab[2] : ab[3]),
        (int)(b & 63));
    const u32 bn = (u32)__builtin_amdgcn_readlane(
        (int)(bq == 0 ? bnq[0] : bq == 1 ? bnq[1] : bq == 2 ? bnq[2]
                                                            : bnq[3]),
        (int)(b & 63));
    const u32 off_in_bucket = tbase - ab_b;
    const u32 tn = (bn > off_in_bucket)
                       ? ((bn - off_in_bucket < (u32)TILE)
                              ? bn - off_in_bucket
                              : (u32)TILE)
                       : 0;
    if (tn == 0) return;   /* block-uniform */

    /* ranks and tile positions two to a register as in the wide form, and
     * so the digits: once the composites are formed the keys are gone */
    u32 pos2[GROUPS / 2] = {};
    u32 dig2[GROUPS / 2] = {};
#pragma unroll
    for (int g = 0; g < GROUPS; ++g) {
        const u32 i = wbase + g * 64 + lane;
        const bool valid = i < tn;
        const u32 d = (u32)(key[g] >> 47) & 511u;
        u32 dlo = 0, dhi = 0;
#pragma unroll
        for (int bit = 0; bit < 9; ++bit) {
            const u32 own = 0u - ((d >> bit) & 1u);
            const u64 bb = __ballot(own != 0);
            dlo |= (u32)bb ^ own;
            dhi |= (u32)(bb >> 32) ^ own;
        }
        const u64 m = __ballot(valid) & ~(((u64)dhi << 32) | dlo);
        const u32 wr = (u32)__popcll(m & ((1ull << lane) - 1ull));
        const u32 before = wc[d];
        pos2[g >> 1] |= (before + wr) << (16 * (g & 1));
        dig2[g >> 1] |= d << (16 * (g & 1));
        if (valid && wr == 0) wc[d] = (u16)(before + (u32)__popcll(m));
        /* the composite, in the key's registers. Formed here and pinned:
         * moved down to its use it would keep the index alive next to the
         * key, and 8 of those do not fit. */
        key[g] = (((key[g] << 17) >> T9_PK_IBITS) << T9_PK_IBITS) |
                 (u64)val[g];
        asm volatile("" : "+v"(key[g]));
    }
    /* and the digits are taken from dig2 again where they are wanted, not
     * kept one to a register from here on */
#pragma unroll
    for (int q = 0; q < GROUPS / 2; ++q)
        asm volatile("" : "+v"(dig2[q]), "+v"(pos2[q]));
    u32 goff = 0;
    if (tid < NDIG9) goff = offs[(u64)tile * NDIG9 + tid];
    __syncthreads();                                   /* A */

    u32 excl = 0;
    if (tid < NDIG9) {
        u32 run = 0;
        for (int w = 0; w < NW; ++w) {
            const u32 c = s_wcnt[w * NDIG9 + tid];
            s_wcnt[w * NDIG9 + tid] = (u16)run;
            run += c;
        }
        u32 v = run;
        for (int off = 1; off < 64; off <<= 1) {
            const u32 y = __shfl_up(v, off);
            if (lane >= (u32)off) v += y;
        }
        excl = v - run;
        if (lane == 63) s_wtot[wave] = v;
    }
    __syncthreads();                                   /* B */
    u32 delta = 0, start = 0;
    if (tid < NDIG9) {
        start = excl;   /* tile position of the digit's run */
        for (u32 w = 0; w < wave; ++w) start += s_wtot[w];
        for (int w = 0; w < NW; ++w)
            s_wcnt[w * NDIG9 + tid] += (u16)start;
        delta = goff - start;
    }
    __syncthreads();                                   /* C */

    /* the one reorder round. The LDS reads run for a whole tile, only the
     * writes are conditional. */
#pragma unroll
    for (int g = 0; g < GROUPS; ++g) {
        const u32 i = wbase + g * 64 + lane;
        const u32 d = (dig2[g >> 1] >> (16 * (g & 1))) & 511u;
        const u32 w = (u32)wc[d];
        const u32 pos = ((pos2[g >> 1] >> (16 * (g & 1))) & 0xffffu) + w;
        if (i < tn) s_ocomp[pos] = key[g];
        pos2[g >> 1] += w << (16 * (g & 1));
    }
    __syncthreads();                                   /* D */
    if (tid < NDIG9) s_delta[tid] = delta;
    if (tid == 256) *s_hi = start;
#pragma unroll
    for (int g = 0; g < GROUPS; ++g) {
        const u32 i = wbase + g * 64 + lane;
        if (i < tn)
            s_dig8[(pos2[g >> 1] >> (16 * (g & 1))) & 0xffffu] =
                (u8)(dig2[g >> 1] >> (16 * (g & 1)));
    }
    __syncthreads();                                   /* E */

    /* slot j = c * 1024 + tid of the reordered tile and its output position
     * (below the end of the output array, as in the wide form). Past tn the
     * digit byte is whatever the counts left there: it indexes s_delta in
     * range and the position is not used. */
    const u32 hi = *s_hi;
    u64 k[GROUPS];
    u32 gpos[GROUPS];
#pragma unroll
    for (int c = 0; c < GROUPS; ++c) k[c] = s_ocomp[c * 1024 + tid];
#pragma unroll
    for (int c = 0; c < GROUPS; ++c) {
        const u32 j = c * 1024 + tid;
        const u32 d = (u32)s_dig8[j] | (j >= hi ? 256u : 0u);
        gpos[c] = s_delta[d] + j;
    }
#pragma unroll
    for (int c = 0; c < GROUPS; ++c)
        if (c * 1024 + tid < tn) out_comp[gpos[c]] = k[c];
}

/* C wrappers so the host flow in t9_sort_msb.hip can launch these
 * without cross-TU template plumbing */
extern "C" {

void t9i_launch_scatter_seg9_packed(u32 grid, void* stream,
                                    const u64* in_keys, const u32* in_vals,
                                    const u32* abase, const u32* bucket_n,
                                    u64* out_comp, const u32* offs) {
    hipLaunchKernelGGL(k_scatter_seg9_packed, dim3(grid), dim3(1024), 0,
                       (hipStream_t)stream, in_keys, in_vals, abase,
                       bucket_n, out_comp, offs);
}

void t9i_launch_hist_seg9(u32 grid, void* stream, const u64* keys,
                          const u32* abase, const u32* bucket_n,
                          u32* hist) {
    hipLaunchKernelGGL(k_hist_seg9, dim3(grid), dim3(256), 0,
                       (hipStream_t)stream, keys, abase, bucket_n, hist);
}

void t9i_launch_seg_scan9(u32 grid, void* stream, u32* hist,
                          const u32* abase, const u32* bucket_n,
                          const u32* true_base, u32* sub_start,
                          u32* sub_n) {
    hipLaunchKernelGGL(k_seg_scan9, dim3(grid), dim3(256), 0,
                       (hipStream_t)stream, hist, abase, bucket_n,
                       true_base, sub_start, sub_n);
}

void t9i_launch_scatter_seg9(u32 grid, int has_val, void* stream,
                             const u64* in_keys, const u32* in_vals,
                             const u32* abase, const u32* bucket_n,
                             u64* out_keys, u32* out_vals,
                             const u32* offs) {
    if (has_val)
        hipLaunchKernelGGL((k_scatter_seg9<true>), dim3(grid), dim3(1024),
                           0, (hipStream_t)stream, in_keys, in_vals, abase,
                           bucket_n, out_keys, out_vals, offs);
    else
        hipLaunchKernelGGL((k_scatter_seg9<false>), dim3(grid), dim3(1024),
                           0, (hipStream_t)stream, in_keys, in_vals, abase,
                           bucket_n, out_keys, out_vals, offs);
}

} /* extern "C" */
