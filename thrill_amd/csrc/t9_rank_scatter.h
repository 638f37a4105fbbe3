/* t9_rank_scatter.h — shared wave-autonomous stable scatter template
 * (included by t9_sort.hip and t9_sort_msb.hip). See t9_sort.hip header
 * comment for the design narrative. */
#pragma once
#include "t9_common.h"

/* exclusive scan of NDIG LDS entries by wave 0 alone (generalized form
 * below; the 256 wrapper keeps existing call sites) */
template <int NDIG>
__device__ inline void t9_scan_onewave(u32* s_vals, u32 tid) {
    if (tid < 64) {
        const u32 lane = tid;
        u32 carry = 0;
        for (int c = 0; c < NDIG / 64; ++c) {
            const u32 v0 = s_vals[c * 64 + lane];
            u32 v = v0;
            for (int off = 1; off < 64; off <<= 1) {
                u32 y = __shfl_up(v, off);
                if (lane >= (u32)off) v += y;
            }
            const u32 total = __shfl(v, 63);
            s_vals[c * 64 + lane] = (v - v0) + carry;
            carry += total;
        }
    }
}

/* exclusive scan of 256 LDS entries by wave 0 alone (4 shfl-scanned
 * 64-lane chunks with a running carry) — replaces the 256-thread
 * Hillis-Steele scan and its 16 block barriers with one. Caller barriers
 * before (values visible to wave 0) and after. */
__device__ inline void t9_scan256_onewave(u32* s_vals, u32 tid) {
    if (tid < 64) {
        const u32 lane = tid;
        u32 carry = 0;
        for (int c = 0; c < 4; ++c) {
            const u32 v0 = s_vals[c * 64 + lane];
            u32 v = v0;
            for (int off = 1; off < 64; off <<= 1) {
                u32 y = __shfl_up(v, off);
                if (lane >= (u32)off) v += y;
            }
            const u32 total = __shfl(v, 63);
            s_vals[c * 64 + lane] = (v - v0) + carry;
            carry += total;
        }
    }
}

/* ballot-combined LDS histogram add: lanes holding the same digit are
 * grouped by BITS ballots; the group leader issues ONE atomicAdd of the
 * group size. Same cost as a plain atomicAdd on uniform digits
 * (memory-bound either way) but immune to the degenerate all-equal-digit
 * case, where 64-way same-address LDS atomics serialize (measured
 * 16x on the segmented hist during the all-identical-records tie
 * bench). */
template <int BITS>
__device__ inline void t9_hist_ballot_add(u32* __restrict__ s_cnt, u32 d,
                                          bool valid, u32 lane) {
    u64 m = __ballot(valid);
    for (int b = 0; b < BITS; ++b) {
        const u64 bb = __ballot((d >> b) & 1u);
        m &= ((d >> b) & 1u) ? bb : ~bb;
    }
    if (valid && (u32)__popcll(m & ((1ull << lane) - 1ull)) == 0)
        atomicAdd(&s_cnt[d], (u32)__popcll(m));
}

/* Wave-autonomous stable scatter of one TILE by BLOCK threads (512 or
 * 1024; the name dates from the first, 512-thread form). In the packed-key
 * forms (REC_WORDS == 0) a lane keeps its keys in registers from the rank
 * loop to the first reorder round: the tile is read from global memory
 * once. The earlier form read it again in round 1 and took that for an
 * L1/L2 hit; the fetch counters put the second read past L2 (DESIGN.md
 * §Measurement, Round 10). */
/* REC_WORDS != 0: "fused extract" mode — in_keys is the packed record
 * array (REC_WORDS u32 words per record); the big-endian u64 key prefix
 * is built from the record bytes and the payload is the record index
 * (iota), eliminating the separate extract pass and the packed key-array
 * round trip for MSB pass 1. */
/* IOTA_VAL: the payload of element base + i is (u32)(base + i) as in the
 * REC_WORDS mode, but the keys are the packed u64 array — pass 1 after the
 * fused extract + histogram, which then need not write the index iota
 * for this kernel to read back (in_vals is not touched). */
/* LDS is what bounds the residency: at the 8192 tile a block holds 74 KiB,
 * so two 1024-thread blocks (8 waves/SIMD) share a CU's 160 KiB and one
 * runs while the other waits on its loads or drains its stores. To fit,
 * the keys, the ranks and tile positions (two to a register) and the
 * output positions live in registers, one u16 array holds the per-wave counts and then, scanned in
 * place, the per-wave offsets, and the keys and then the values are
 * reordered through the same buffer. */
template <int TILE, int BLOCK, bool HAS_KEY, bool HAS_VAL,
          int REC_WORDS = 0, bool IOTA_VAL = false>
__global__ __launch_bounds__(BLOCK, 8) void k_scatter_wave512(
    const u64* __restrict__ in_keys, const u32* __restrict__ in_vals,
    u64* __restrict__ out_keys, u32* __restrict__ out_vals,
    const u32* __restrict__ offs, u64 n, u32 shift) {
    constexpr int NW = BLOCK / 64;
    constexpr int SUB = TILE / NW;
    constexpr int GROUPS = SUB / 64;   /* = TILE / BLOCK: elements per lane */
    static_assert(HAS_KEY, "the store phase reads the digit from the key");
    static_assert(TILE % BLOCK == 0 && SUB % 64 == 0, "whole groups");
    static_assert(GROUPS % 2 == 0, "positions are kept two to a register");
    const u32* rec32 = (const u32*)in_keys;
    /* keys in round 1, values in round 2 (bytes: may alias both) */
    __shared__ __align__(16) u8 s_raw[TILE * 8];
    u64* const s_okeys = (u64*)s_raw;
    u32* const s_ovals = (u32*)s_raw;
    /* per wave and digit: first the count (<= SUB, a wave's sub-tile),
     * then the elements of that digit in the waves before (<= TILE - SUB);
     * a rank is < SUB and a tile position < TILE. All fit 16 bits. */
    static_assert(TILE <= 65535, "u16 counts and offsets");
    __shared__ u16 s_wcnt[NW * T9_RADIX];
    __shared__ u32 s_start[T9_RADIX];
    __shared__ u32 s_goff[T9_RADIX];

    const u32 tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    /* Which tile: blocks are dealt to the 8 XCDs in turn, so block b and
     * b + 8 share an L2. Each XCD takes a contiguous eighth of the tiles
     * (the remainder goes to the first XCDs), as in k_scatter_seg9: tiles
     * t and t + 1 append neighbouring runs to every bucket, and the line
     * on which two such runs meet is then written from one L2. Any
     * bijection is correct; base, tn and the offs row follow the tile. */
    const u32 xper = gridDim.x >> 3, xrem = gridDim.x & 7;
    const u32 xcd = blockIdx.x & 7;
    const u32 tile = xcd * xper + (xcd < xrem ? xcd : xrem) +
                     (blockIdx.x >> 3);
    const u64 base = (u64)tile * TILE;
    const u32 tn = (u32)((n - base < (u64)TILE) ? (n - base) : (u64)TILE);

    /* Every key is read from global memory once (a second read of the tile
     * went past L2: 64 tiles of 64 KiB in flight per XCD are the whole
     * 4 MiB). One round of unconditional loads, all in flight before the
     * first ballot: a lane past the end of a ragged tile reads the tile's
     * last key, which takes no part in the match or in the counts. */
    constexpr bool ONE_READ = !REC_WORDS;
    constexpr bool LOAD_VAL = HAS_VAL && !REC_WORDS && !IOTA_VAL;
    const u32 wbase = wave * SUB;
    u64 key[ONE_READ ? GROUPS : 1];
    u32 val[LOAD_VAL ? GROUPS : 1];
    if constexpr (ONE_READ) {
#pragma unroll
        for (int g = 0; g < GROUPS; ++g) {
            const u32 i = wbase + g * 64 + lane;
            key[g] = in_keys[base + (i < tn ? i : tn - 1)];
        }
        if constexpr (LOAD_VAL) {
#pragma unroll
            for (int g = 0; g < GROUPS; ++g) {
                const u32 i = wbase + g * 64 + lane;
                val[g] = in_vals[base + (i < tn ? i : tn - 1)];
            }
        }
    }

    if (tid < T9_RADIX)
        s_goff[tid] = offs[(u64)tile * T9_RADIX + tid];
    u16* const wc = s_wcnt + wave * T9_RADIX;
    for (u32 t = lane; t < T9_RADIX; t += 64) wc[t] = 0;

    /* rank inside the wave's sub-tile, then position inside the tile; ranks
     * (<= SUB) and tile positions (< TILE) two to a register */
    u32 pos2[GROUPS / 2] = {};
#pragma unroll
    for (int g = 0; g < GROUPS; ++g) {
        const u32 i = wbase + g * 64 + lane;
        const bool valid = i < tn;
        u32 d = 0;
        if constexpr (ONE_READ) {
            d = (u32)(key[g] >> shift) & 255u;
        }
        else if (valid) {
            if (REC_WORDS)
                d = ((const u8*)rec32)[(base + i) * (u64)REC_WORDS * 4 +
                                       (7 - shift / 8)];
            else
                d = (u32)(in_keys[base + i] >> shift) & 255u;
        }
        u64 m = __ballot(valid);
        for (int bit = 0; bit < 8; ++bit) {
            u64 bb = __ballot((d >> bit) & 1u);
            m &= ((d >> bit) & 1u) ? bb : ~bb;
        }
        const u32 wr = (u32)__popcll(m & ((1ull << lane) - 1ull));
        const u32 before = valid ? (u32)wc[d] : 0;
        pos2[g >> 1] |= (before + wr) << (16 * (g & 1));
        if (valid && wr == 0) wc[d] = (u16)(before + (u32)__popcll(m));
    }
    /* the digits and their count addresses are formed again from the keys
     * in round 1, not carried there one to a register next to the keys */
    if constexpr (ONE_READ) {
#pragma unroll
        for (int g = 0; g < GROUPS; ++g) asm volatile("" : "+v"(key[g]));
#pragma unroll
        for (int q = 0; q < GROUPS / 2; ++q) asm volatile("" : "+v"(pos2[q]));
    }
    __syncthreads();

    /* combine (threads 0..255 own digit tid): counts -> offsets in place */
    if (tid < T9_RADIX) {
        u32 run = 0;
        for (int w = 0; w < NW; ++w) {
            const u32 c = s_wcnt[w * T9_RADIX + tid];
            s_wcnt[w * T9_RADIX + tid] = (u16)run;
            run += c;
        }
        s_start[tid] = run;
    }
    __syncthreads();
    t9_scan256_onewave(s_start, tid);   /* s_start: totals -> exclusive */
    __syncthreads();

    /* round 1: keys. A lane past tn adds nothing to its half of pos2, so
     * the other half is left alone. */
#pragma unroll
    for (int g = 0; g < GROUPS; ++g) {
        const u32 i = wbase + g * 64 + lane;
        if (i < tn) {
            u64 k;
            if constexpr (ONE_READ) {
                k = key[g];
            }
            else if (REC_WORDS) {
                const u64 w0 = (u64)rec32[(base + i) * REC_WORDS];
                const u64 w1 = (u64)rec32[(base + i) * REC_WORDS + 1];
                k = ((u64)__builtin_bswap32((u32)w0) << 32) |
                    __builtin_bswap32((u32)w1);
            }
            else {
                k = in_keys[base + i];
            }
            if constexpr (LOAD_VAL && !ONE_READ) val[g] = in_vals[base + i];
            const u32 d = (u32)(k >> shift) & 255u;
            const u32 add = s_start[d] + (u32)wc[d];
            const u32 pos = ((pos2[g >> 1] >> (16 * (g & 1))) & 0xffffu) + add;
            s_okeys[pos] = k;
            pos2[g >> 1] += add << (16 * (g & 1));
        }
    }
    __syncthreads();

    /* an output position is below the end of the output array, which the
     * u32 offsets in offs already address */
    u32 gpos[GROUPS];
#pragma unroll
    for (int c = 0; c < GROUPS; ++c) {
        const u32 j = c * BLOCK + tid;
        if (j < tn) {
            const u64 k = s_okeys[j];
            const u32 d = (u32)(k >> shift) & 255u;
            gpos[c] = s_goff[d] + (j - s_start[d]);
            out_keys[gpos[c]] = k;
        }
    }
    if (!HAS_VAL) return;
    __syncthreads();

    /* round 2: values, through the same buffer */
#pragma unroll
    for (int g = 0; g < GROUPS; ++g) {
        const u32 i = wbase + g * 64 + lane;
        if (i < tn) {
            const u32 pos = (pos2[g >> 1] >> (16 * (g & 1))) & 0xffffu;
            if constexpr (LOAD_VAL) s_ovals[pos] = val[g];
            else s_ovals[pos] = (u32)(base + i);
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < GROUPS; ++c) {
        const u32 j = c * BLOCK + tid;
        if (j < tn) out_vals[gpos[c]] = s_ovals[j];
    }
}

