/* t9_text.hip — real text on the device: tokenizer, string hasher and the
 * first-occurrence pick that lets word_count run on raw bytes.
 *
 * Semantics are the reference pipeline's: ReadLines splits at '\n'
 * (thrill/api/read_lines.hpp), WordCount splits each line at ' ' and drops
 * empty words (examples/word_count/word_count.hpp:37-45). So a token is a
 * maximal run of bytes that are neither 0x20 nor 0x0A; every other byte
 * value (0x00, '\t', '\r', 0x80-0xFF) is a word byte, and a token running
 * to the end of the buffer is a token.
 *
 * Tokenizer = the repository's compaction shape (t9_group.hip): per-tile
 * count -> single-block scan of the tile summaries -> scatter. Flags need
 * only the byte BEFORE a position:
 *   start(j) = word(j)  && (j == 0 || delim(j-1))
 *   stop(j)  = delim(j) && j > 0 && word(j-1)      (j == nbytes is a delim)
 * stop(j) is the exclusive end of a token, so positions 0..nbytes are
 * scanned (one virtual delimiter past the buffer closes a trailing token).
 * The k-th start and the k-th stop belong to the same token. Stops are
 * RANKED (exclusive prefix sum -> token index); starts are CARRIED (running
 * maximum of "last start position seen" -> the open token's offset). Both
 * scans run in the same pass, so the lane that finds a stop holds the
 * token's index, offset and length at once (ranking both flag sets would
 * leave len[k] needing off[k] from another lane: a third pass). Nobody
 * walks forward to a delimiter, a megabyte-long token costs the same as any
 * other, and a tile boundary is crossed by two u32 per tile.
 *
 * Hasher = FNV-1a under two bases, a serial chain per token: one lane per
 * token, both chains advanced together, bytes fetched as aligned 8-byte
 * words (byte loads only in the last partial word of the buffer).
 */

#include "t9_common.h"

#define TXT_THREADS 256
#define TXT_ROW (TXT_THREADS * 16)      /* bytes per block-wide 16-B load */
#define TXT_ROWS 8
#define TXT_TILE (TXT_ROW * TXT_ROWS)   /* 32 KiB of text per block */

/* 0x80 in every byte of v that is zero (exact, no borrow artefacts) */
__host__ __device__ inline u32 txt_zero_bytes(u32 v) {
    return ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v | 0x7F7F7F7Fu);
}

/* bit i = byte i of w (lowest address first) is ' ' or '\n' */
__host__ __device__ inline u32 txt_delim4(u32 w) {
    const u32 m = txt_zero_bytes(w ^ 0x20202020u) |
                  txt_zero_bytes(w ^ 0x0A0A0A0Au);
    /* gather bits 7,15,23,31 into a nibble: the partial products land on
     * distinct bits, so nothing carries */
    return (((m >> 7) * 0x01020408u) >> 24) & 0xFu;
}

__host__ __device__ inline u32 txt_delim16(uint4 v) {
    return txt_delim4(v.x) | (txt_delim4(v.y) << 4) |
           (txt_delim4(v.z) << 8) | (txt_delim4(v.w) << 12);
}

/* the 16 bytes at text[g..g+16), positions >= n read as ' ' (never
 * touched): one 16-byte load when the chunk is inside the buffer, byte
 * loads for the unaligned tail */
__device__ inline uint4 txt_load16(const u8* __restrict__ text, u64 g,
                                   u64 n) {
    if (g + 16 <= n) return *reinterpret_cast<const uint4*>(text + g);
    u32 w0 = 0x20202020u, w1 = w0, w2 = w0, w3 = w0;
    if (g < n) {
#pragma unroll
        for (u32 i = 0; i < 16; ++i) {
            if (g + i < n) {
                const u32 sh = 8 * (i & 3);
                const u32 b = (u32)text[g + i] << sh;
                const u32 keep = ~(0xFFu << sh);
                if ((i >> 2) == 0) w0 = (w0 & keep) | b;
                else if ((i >> 2) == 1) w1 = (w1 & keep) | b;
                else if ((i >> 2) == 2) w2 = (w2 & keep) | b;
                else w3 = (w3 & keep) | b;
            }
        }
    }
    return make_uint4(w0, w1, w2, w3);
}

/* start/stop flag masks of the 16 positions g..g+15. The byte before the
 * chunk comes from the neighbouring lane's mask; lane 0 of a wave reads
 * the one byte itself (in bounds: 0 < g <= n). */
__device__ inline void txt_flags(const u8* __restrict__ text, u64 g, u64 n,
                                 u32* starts, u32* stops) {
    const u32 d = txt_delim16(txt_load16(text, g, n));
    const u32 lane = threadIdx.x & (T9_WAVE - 1);
    u32 prev = (u32)__shfl_up((int)(d >> 15), 1);
    if (lane == 0) {
        prev = 1;
        if (g > 0 && g <= n) {
            const u8 c = text[g - 1];
            prev = (c == 0x20 || c == 0x0A) ? 1u : 0u;
        }
    }
    const u32 pd = ((d << 1) | prev) & 0xFFFFu;
    *starts = ~d & pd & 0xFFFFu;
    *stops = d & ~pd & 0xFFFFu;
}

/* per tile: number of stops, and 1 + position of the last start (0 = the
 * tile has none) */
__global__ __launch_bounds__(TXT_THREADS) void k_txt_count(
    const u8* __restrict__ text, u64 n, uint2* __restrict__ tiles) {
    __shared__ u32 s_cnt;
    __shared__ u32 s_last;
    if (threadIdx.x == 0) {
        s_cnt = 0;
        s_last = 0;
    }
    __syncthreads();
    const u64 base = (u64)blockIdx.x * TXT_TILE + (u64)threadIdx.x * 16;
    u32 cnt = 0, last = 0;
#pragma unroll
    for (u32 r = 0; r < TXT_ROWS; ++r) {
        const u64 g = base + (u64)r * TXT_ROW;
        u32 st, sp;
        txt_flags(text, g, n, &st, &sp);
        cnt += __popc(sp);
        if (st) last = (u32)g + (31 - __clz(st)) + 1;   /* rows ascend */
    }
    for (int o = T9_WAVE / 2; o > 0; o >>= 1) {
        cnt += (u32)__shfl_down((int)cnt, o);
        const u32 y = (u32)__shfl_down((int)last, o);
        last = last > y ? last : y;
    }
    if ((threadIdx.x & (T9_WAVE - 1)) == 0) {
        atomicAdd(&s_cnt, cnt);
        atomicMax(&s_last, last);
    }
    __syncthreads();
    if (threadIdx.x == 0) tiles[blockIdx.x] = make_uint2(s_cnt, s_last);
}

/* exclusive (sum, max) scan of the B tile summaries, in place; one block,
 * each thread owns a contiguous slice */
__global__ __launch_bounds__(256) void k_txt_scan(uint2* __restrict__ tiles,
                                                  u32 B,
                                                  u64* __restrict__ total) {
    __shared__ u32 s_sum[256];
    __shared__ u32 s_max[256];
    const u32 tid = threadIdx.x;
    const u32 per = (B + 255) / 256;
    const u32 b0 = tid * per;
    const u32 b1 = (b0 + per < B) ? b0 + per : B;
    u32 sum = 0, mx = 0;
    for (u32 i = b0; i < b1; ++i) {
        const uint2 t = tiles[i];
        sum += t.x;
        mx = mx > t.y ? mx : t.y;
    }
    s_sum[tid] = sum;
    s_max[tid] = mx;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const u32 ys = (tid >= (u32)off) ? s_sum[tid - off] : 0;
        const u32 ym = (tid >= (u32)off) ? s_max[tid - off] : 0;
        __syncthreads();
        s_sum[tid] += ys;
        s_max[tid] = s_max[tid] > ym ? s_max[tid] : ym;
        __syncthreads();
    }
    u32 run_sum = s_sum[tid] - sum;               /* exclusive */
    u32 run_max = tid ? s_max[tid - 1] : 0;
    for (u32 i = b0; i < b1; ++i) {
        const uint2 t = tiles[i];
        tiles[i] = make_uint2(run_sum, run_max);
        run_sum += t.x;
        run_max = run_max > t.y ? run_max : t.y;
    }
    if (tid == 255) *total = s_sum[255];
}

/* Scatter: ranks and open-token offsets per row as described above; the
 * row's tokens are staged in LDS at their row-local rank and written out
 * by the whole block as contiguous runs (a lane's own tokens are ~3 ranks
 * apart from its neighbour's, so direct stores would touch each output
 * line from several instructions). Staging and wave totals are
 * double-buffered by row parity: two barriers per row. */
__global__ __launch_bounds__(TXT_THREADS) void k_txt_scatter(
    const u8* __restrict__ text, u64 n, const uint2* __restrict__ tiles,
    u32* __restrict__ tok_off, u32* __restrict__ tok_len) {
    __shared__ u32 s_wsum[2][TXT_THREADS / T9_WAVE];
    __shared__ u32 s_wmax[2][TXT_THREADS / T9_WAVE];
    __shared__ u32 s_off[2][TXT_ROW / 2];   /* a row closes <= ROW/2 tokens */
    __shared__ u32 s_len[2][TXT_ROW / 2];
    const u32 lane = threadIdx.x & (T9_WAVE - 1);
    const u32 wave = threadIdx.x / T9_WAVE;
    const uint2 tb = tiles[blockIdx.x];
    u32 rank0 = tb.x;   /* tokens closed before this row */
    u32 open0 = tb.y;   /* 1 + last start before this row */
    const u64 base = (u64)blockIdx.x * TXT_TILE + (u64)threadIdx.x * 16;
    for (u32 r = 0; r < TXT_ROWS; ++r) {
        const u64 g = base + (u64)r * TXT_ROW;
        u32 st, sp;
        txt_flags(text, g, n, &st, &sp);
        const u32 cnt = __popc(sp);
        const u32 last = st ? (u32)g + (31 - __clz(st)) + 1 : 0;
        u32 isum = cnt, imax = last;   /* inclusive wave scans */
        for (int o = 1; o < T9_WAVE; o <<= 1) {
            const u32 ys = (u32)__shfl_up((int)isum, o);
            const u32 ym = (u32)__shfl_up((int)imax, o);
            if (lane >= (u32)o) {
                isum += ys;
                imax = imax > ym ? imax : ym;
            }
        }
        u32 emax = (u32)__shfl_up((int)imax, 1);
        if (lane == 0) emax = 0;
        const u32 par = r & 1;
        if (lane == T9_WAVE - 1) {
            s_wsum[par][wave] = isum;
            s_wmax[par][wave] = imax;
        }
        __syncthreads();
        u32 lrank = isum - cnt;   /* row-local rank of this lane's 1st stop */
        u32 open = open0 > emax ? open0 : emax;
        u32 row_sum = 0, row_max = 0;
#pragma unroll
        for (u32 w = 0; w < TXT_THREADS / T9_WAVE; ++w) {
            const u32 ws = s_wsum[par][w], wm = s_wmax[par][w];
            if (w < wave) {
                lrank += ws;
                open = open > wm ? open : wm;
            }
            row_sum += ws;
            row_max = row_max > wm ? row_max : wm;
        }
        /* walk this lane's flags in text order: a start opens a token, a
         * stop closes the open one at the stop's rank */
        u32 m = st | sp;
        while (m) {
            const u32 b = __ffs(m) - 1;
            m &= m - 1;
            const u32 pos = (u32)g + b;
            if ((st >> b) & 1) {
                open = pos + 1;
            }
            else {
                s_off[par][lrank] = open - 1;
                s_len[par][lrank] = pos - (open - 1);
                ++lrank;
            }
        }
        __syncthreads();
        for (u32 i = threadIdx.x; i < row_sum; i += TXT_THREADS) {
            tok_off[rank0 + i] = s_off[par][i];
            tok_len[rank0 + i] = s_len[par][i];
        }
        rank0 += row_sum;
        open0 = open0 > row_max ? open0 : row_max;
    }
}

/* one lane per token; h1/h2 are the two FNV-1a chains of
 * detail::string_hash2 (include/t9/dia.hpp), mixed by Hash128to64 */
__global__ __launch_bounds__(256) void k_txt_hash2(
    const u8* __restrict__ text, u64 nbytes, const u32* __restrict__ off,
    const u32* __restrict__ len, u64 n, u64* __restrict__ k1,
    u64* __restrict__ k2, u32* __restrict__ err) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 beg = off[i];
    const u64 end = beg + len[i];
    if (end > nbytes) {   /* caller error: report, do not read */
        atomicExch(err, 1u);
        k1[i] = 0;
        k2[i] = 0;
        return;
    }
    const u64 P = 0x100000001B3ull;
    u64 h1 = 0xCBF29CE484222325ull, h2 = 0x84222325CBF29CE4ull;
    const u64* __restrict__ words = reinterpret_cast<const u64*>(text);
    u64 pos = beg;
    while (pos < end) {
        const u64 wb = pos & ~(u64)7;
        u64 w;
        if (wb + 8 <= nbytes) {
            w = words[wb >> 3];
        }
        else {   /* last partial word of the buffer */
            w = 0;
            for (u64 j = pos; j < end; ++j)
                w |= (u64)text[j] << (8 * (j - wb));
        }
        const u32 lo = (u32)(pos - wb);
        const u32 hi = (end - wb < 8) ? (u32)(end - wb) : 8u;
        w >>= 8 * lo;
        for (u32 j = lo; j < hi; ++j) {
            const u64 b = w & 0xFF;
            w >>= 8;
            h1 = (h1 ^ b) * P;
            h2 = (h2 ^ b) * P;
        }
        pos = wb + hi;
    }
    u64 a = t9_hash128to64(0x9AE16A3B2F90404Full, h1);
    u64 b = t9_hash128to64(0xC3A5C85C97CB3127ull, h2);
    if (a == ~0ull) a ^= 1;   /* reserved table sentinels */
    if (b == ~0ull) b ^= 1;
    k1[i] = a;
    k2[i] = b;
}

/* first[s] = min token index mapped to slot s. The plain read skips the
 * atomic when the stored index is already smaller (the table's
 * read-before-CAS idiom): tokens of a hot word arrive roughly in order,
 * so nearly all of them skip. */
__global__ __launch_bounds__(256) void k_txt_first(
    const u32* __restrict__ slot, u64 n, u32* __restrict__ first,
    u64 cap) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u32 s = slot[i];
    if (s == 0xFFFFFFFFu || (u64)s >= cap) return;
    const u32 me = (u32)i;
    if (__atomic_load_n(&first[s], __ATOMIC_RELAXED) > me)
        atomicMin(&first[s], me);
}

namespace {
u64 txt_tiles(u64 nbytes) { return nbytes / TXT_TILE + 1; }  /* 0..nbytes */
} // namespace

extern "C" {

u64 t9_text_tokenize_workspace(u64 nbytes) {
    return t9_align256(txt_tiles(nbytes) * sizeof(uint2));
}

int t9_text_tokenize(t9_context* ctx, const u8* d_text, u64 nbytes,
                     u32* d_tok_off, u32* d_tok_len, u64* d_ntok,
                     void* d_workspace, void* stream) {
    (void)ctx;
    if (nbytes >= (1ull << 32)) return T9_EINVAL;
    if (!d_ntok || !d_workspace) return T9_EINVAL;
    if ((d_tok_off == nullptr) != (d_tok_len == nullptr)) return T9_EINVAL;
    if (nbytes && (!d_text || ((uintptr_t)d_text & 15))) return T9_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_ntok, 0, 8, s));
    if (nbytes == 0) return T9_OK;
    const u32 B = (u32)txt_tiles(nbytes);
    uint2* tiles = (uint2*)d_workspace;
    hipLaunchKernelGGL(k_txt_count, dim3(B), dim3(TXT_THREADS), 0, s,
                       d_text, nbytes, tiles);
    hipLaunchKernelGGL(k_txt_scan, dim3(1), dim3(256), 0, s, tiles, B,
                       d_ntok);
    if (d_tok_off)
        hipLaunchKernelGGL(k_txt_scatter, dim3(B), dim3(TXT_THREADS), 0, s,
                           d_text, nbytes, tiles, d_tok_off, d_tok_len);
    T9_LAUNCH_CHECK();
    return T9_OK;
}

int t9_text_hash2(t9_context* ctx, const u8* d_text, u64 nbytes,
                  const u32* d_off, const u32* d_len, u64 n, u64* d_k1,
                  u64* d_k2, u32* d_error, void* stream) {
    (void)ctx;
    if (!d_error) return T9_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_error, 0, 4, s));
    if (n == 0) return T9_OK;
    if (!d_off || !d_len || !d_k1 || !d_k2) return T9_EINVAL;
    if (nbytes && (!d_text || ((uintptr_t)d_text & 7))) return T9_EINVAL;
    const u64 blocks = t9_ceil_div(n, 256);
    if (blocks >= (1ull << 31)) return T9_EINVAL;
    hipLaunchKernelGGL(k_txt_hash2, dim3((u32)blocks), dim3(256), 0, s,
                       d_text, nbytes, d_off, d_len, n, d_k1, d_k2,
                       d_error);
    T9_LAUNCH_CHECK();
    return T9_OK;
}

int t9_text_first_token(t9_context* ctx, const u32* d_slot, u64 n,
                        u32* d_first, u64 capacity, void* stream) {
    (void)ctx;
    if (n >= (1ull << 32)) return T9_EINVAL;
    if (capacity && !d_first) return T9_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (capacity) HIP_TRY(hipMemsetAsync(d_first, 0xFF, capacity * 4, s));
    if (n == 0 || capacity == 0) return T9_OK;
    if (!d_slot) return T9_EINVAL;
    hipLaunchKernelGGL(k_txt_first, dim3((u32)t9_ceil_div(n, 256)),
                       dim3(256), 0, s, d_slot, n, d_first, capacity);
    T9_LAUNCH_CHECK();
    return T9_OK;
}

} /* extern "C" */
