/* t9_scan.hip — device prefix scan and whole-array fold with a selectable
 * operator (SUM / MIN / MAX) over u64, i64 and f64 values, gfx950.
 *
 * The reference's PrefixSum / ExPrefixSum (api/prefix_sum.hpp:92-110) with
 * ⊕ the operator and `initial` a 64-bit pattern:
 *   inclusive: out[i] = initial ⊕ x[0] ⊕ … ⊕ x[i]
 *   exclusive: out[0] = initial, out[i] = initial ⊕ x[0] ⊕ … ⊕ x[i-1]
 * Operators and value types are those of t9_reduce_op.hip: SUM is the
 * wrapping 64-bit add on the raw bits; MIN and MAX compare as unsigned
 * after the order-preserving encoding t9_enc (applied at load, undone at
 * store), so the kernels see one unsigned compare and every result is
 * bit-exact however the work is split. SUM over F64 is refused.
 *
 * Three launches, and no block ever waits on another block:
 *   1. tile fold     one block per tile of T9_SCAN_TILE elements writes the
 *                    (encoded) fold of its tile to partial[b];
 *   2. partials scan exclusive scan of the partials seeded with `initial`,
 *                    in place. Up to T9_SCAN_PART partials: one block, wave
 *                    scans in registers. More: a second level of the same
 *                    shape — fold the partials in tiles of T9_SCAN_PART,
 *                    scan those block totals in one block (it loops, so
 *                    any count is correct), scan each tile of partials
 *                    from its carry — so that the partials of a 2^28
 *                    element array (65 536 of them) are scanned by 128
 *                    blocks, not by one (cf. T9_SCAN_CHUNK in t9_common.h);
 *   3. tile scan     each block re-reads its own tile, scans it from its
 *                    carry and writes the output (d_out == d_in is fine:
 *                    a block reads nothing but its own tile).
 *
 * Inside a block: 16-byte global accesses (two u64 or one {key, value}
 * pair per lane), the per-wave scan in registers by shuffles, ONE LDS
 * exchange of the 4 x ROUNDS wave totals per chunk of rounds, and a
 * running carry across the rounds and chunks of a tile.
 *
 * A single-pass chained scan (decoupled look-back) would save one of the
 * three 8 B/element transfers but needs blocks that spin on their
 * predecessors; it is deliberately not built here.
 */

#include "t9_common.h"
#include "thrill_amd.h"

#include <cstdlib>

#define T9_SCAN_TILE 4096u   /* elements per block of pass 1 and pass 3 */
#define T9_SCAN_PART 512u    /* partials per block of pass 2 */
#define T9_FOLD_GRID 2048u   /* most blocks of a stand-alone fold */

namespace {

enum { L_U64 = 0, L_KV = 1 };

template <int OP>
__device__ __forceinline__ u64 sc_comb(u64 a, u64 b) {
    if (OP == T9_OP_SUM) return a + b;
    if (OP == T9_OP_MIN) return a < b ? a : b;
    return a < b ? b : a;
}

/* the operator's identity in the encoded domain */
template <int OP>
__host__ __device__ constexpr u64 sc_ident() {
    return OP == T9_OP_MIN ? ~0ull : 0ull;
}

/* inclusive scan across the 64 lanes of a wave */
template <int OP>
__device__ __forceinline__ u64 sc_wave_scan(u64 v, u32 lane) {
#pragma unroll
    for (u32 off = 1; off < 64; off <<= 1) {
        const u64 y = __shfl_up((unsigned long long)v, off, 64);
        if (lane >= off) v = sc_comb<OP>(v, y);
    }
    return v;
}

/* fold across the 64 lanes of a wave; every lane gets the result */
template <int OP>
__device__ __forceinline__ u64 sc_wave_fold(u64 v) {
#pragma unroll
    for (u32 off = 32; off; off >>= 1)
        v = sc_comb<OP>(v, (u64)__shfl_xor((unsigned long long)v, off, 64));
    return v;
}

/* elements one 16-byte access per lane of a 256-thread block covers */
template <int LAYOUT>
__host__ __device__ constexpr u32 sc_epr() {
    return LAYOUT == L_U64 ? 512u : 256u;
}

/* One 16-byte access of lane-slot i. L_U64: elements i and i+1 into
 * (a, b). L_KV: pair i, key into a and value into b. Values come back
 * encoded; what lies past n is the identity. `vec` is false only for a
 * base pointer that is not 16-byte aligned. */
template <int OP, int LAYOUT>
__device__ __forceinline__ void sc_load(const u64* in, u64 i, u64 n,
                                        int vtype, bool vec, u64& a,
                                        u64& b) {
    if (LAYOUT == L_U64) {
        if (vec && i + 1 < n) {
            const ulonglong2 v = *(const ulonglong2*)(in + i);
            a = t9_enc(v.x, OP, vtype);
            b = t9_enc(v.y, OP, vtype);
        }
        else {
            a = i < n ? t9_enc(in[i], OP, vtype) : sc_ident<OP>();
            b = i + 1 < n ? t9_enc(in[i + 1], OP, vtype) : sc_ident<OP>();
        }
    }
    else {
        a = 0;
        b = sc_ident<OP>();
        if (i < n) {
            if (vec) {
                const ulonglong2 v = *(const ulonglong2*)(in + 2 * i);
                a = v.x;
                b = t9_enc(v.y, OP, vtype);
            }
            else {
                a = in[2 * i];
                b = t9_enc(in[2 * i + 1], OP, vtype);
            }
        }
    }
}

/* the mirror of sc_load: (a, b) are final (decoded) words */
template <int LAYOUT>
__device__ __forceinline__ void sc_store(u64* out, u64 i, u64 n, bool vec,
                                         u64 a, u64 b) {
    if (LAYOUT == L_U64) {
        if (vec && i + 1 < n) {
            *(ulonglong2*)(out + i) = make_ulonglong2(a, b);
        }
        else {
            if (i < n) out[i] = a;
            if (i + 1 < n) out[i + 1] = b;
        }
    }
    else if (i < n) {
        if (vec) {
            *(ulonglong2*)(out + 2 * i) = make_ulonglong2(a, b);
        }
        else {
            out[2 * i] = a;
            out[2 * i + 1] = b;
        }
    }
}

} // namespace

/* Pass 1 and the stand-alone fold. Block b folds tile t0, t0 + grid, …
 * and writes one encoded word. With grid == number of tiles each block has
 * exactly one tile; `rev` then makes block b take tile nt-1-b (and write
 * partial[nt-1-b]), so that the tiles read last are the ones pass 3 reads
 * first. */
template <int OP, int LAYOUT, u32 ROUNDS>
__global__ __launch_bounds__(256) void k_scan_fold(
    const u64* __restrict__ in, u64 n, u64 nt, int vtype, int vec, int rev,
    u64* __restrict__ partial) {
    __shared__ u64 s_w[4];
    constexpr u32 EPR = sc_epr<LAYOUT>();
    const u32 tid = threadIdx.x;
    const u64 t0 = rev ? nt - 1 - blockIdx.x : (u64)blockIdx.x;
    u64 acc = sc_ident<OP>();
    for (u64 t = t0; t < nt; t += gridDim.x) {
        const u64 base = t * (u64)(EPR * ROUNDS);
        u64 a[ROUNDS], b[ROUNDS];
#pragma unroll
        for (u32 r = 0; r < ROUNDS; ++r)
            sc_load<OP, LAYOUT>(in,
                                base + r * EPR +
                                    (LAYOUT == L_U64 ? 2 * tid : tid),
                                n, vtype, vec != 0, a[r], b[r]);
#pragma unroll
        for (u32 r = 0; r < ROUNDS; ++r) {
            if (LAYOUT == L_U64) acc = sc_comb<OP>(acc, a[r]);
            acc = sc_comb<OP>(acc, b[r]);
        }
    }
    acc = sc_wave_fold<OP>(acc);
    if ((tid & 63) == 0) s_w[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0)
        partial[rev ? t0 : (u64)blockIdx.x] = sc_comb<OP>(
            sc_comb<OP>(s_w[0], s_w[1]), sc_comb<OP>(s_w[2], s_w[3]));
}

/* Pass 3 (and the tile level of pass 2): scan one tile from carry[b].
 * A tile is CHUNKS chunks of ROUNDS rounds; the rounds of a chunk sit in
 * registers, their wave totals cross the block in one LDS exchange
 * (double-buffered, so one barrier per chunk), `run` carries on. */
template <int OP, int LAYOUT, u32 ROUNDS, u32 CHUNKS, bool EXCL>
__global__ __launch_bounds__(256) void k_scan_tile(
    const u64* in, u64* out, u64 n, const u64* __restrict__ carry,
    int vtype, int vec) {
    __shared__ u64 s_tot[2][ROUNDS * 4];
    constexpr u32 EPR = sc_epr<LAYOUT>();
    const u32 tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const u64 tile0 = (u64)blockIdx.x * (u64)(EPR * ROUNDS * CHUNKS);
    const u32 mine = LAYOUT == L_U64 ? 2 * tid : tid;
    u64 run = carry[blockIdx.x];
    for (u32 c = 0; c < CHUNKS; ++c) {
        const u64 base = tile0 + (u64)c * (EPR * ROUNDS);
        if (base >= n) break;   /* block-uniform */
        u64 a[ROUNDS], b[ROUNDS], ex[ROUNDS];
#pragma unroll
        for (u32 r = 0; r < ROUNDS; ++r)
            sc_load<OP, LAYOUT>(in, base + r * EPR + mine, n, vtype,
                                vec != 0, a[r], b[r]);
#pragma unroll
        for (u32 r = 0; r < ROUNDS; ++r) {
            const u64 v = LAYOUT == L_U64 ? sc_comb<OP>(a[r], b[r]) : b[r];
            const u64 s = sc_wave_scan<OP>(v, lane);
            const u64 up = __shfl_up((unsigned long long)s, 1, 64);
            ex[r] = lane ? up : sc_ident<OP>();
            if (lane == 63) s_tot[c & 1][r * 4 + w] = s;
        }
        __syncthreads();
#pragma unroll
        for (u32 r = 0; r < ROUNDS; ++r) {
            u64 pre = run;
#pragma unroll
            for (u32 k = 0; k < 4; ++k) {
                const u64 t = s_tot[c & 1][r * 4 + k];
                if (k < w) pre = sc_comb<OP>(pre, t);
                run = sc_comb<OP>(run, t);
            }
            /* everything before this lane's first element */
            const u64 p = sc_comb<OP>(pre, ex[r]);
            u64 o0, o1;
            if (LAYOUT == L_U64) {
                const u64 pa = sc_comb<OP>(p, a[r]);
                o0 = t9_dec(EXCL ? p : pa, OP, vtype);
                o1 = t9_dec(EXCL ? pa : sc_comb<OP>(pa, b[r]), OP, vtype);
            }
            else {
                o0 = a[r];
                o1 = t9_dec(sc_comb<OP>(p, b[r]), OP, vtype);
            }
            sc_store<LAYOUT>(out, base + r * EPR + mine, n, vec != 0, o0,
                             o1);
        }
    }
}

/* Top of pass 2: ONE block scans p[0..cnt) in place, exclusive, seeded
 * with init (all encoded words); it loops, so any cnt is correct. The
 * fold of all of them WITHOUT init goes, decoded, to *total if non-NULL. */
template <int OP>
__global__ __launch_bounds__(256) void k_scan_top(
    u64* __restrict__ p, u64 cnt, u64 init, int vtype,
    u64* __restrict__ total) {
    __shared__ u64 s_tot[2][4];
    const u32 tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    u64 run = sc_ident<OP>();
    u32 buf = 0;
    for (u64 base = 0; base < cnt; base += 512, buf ^= 1) {
        const u64 i = base + 2 * tid;
        const u64 a = i < cnt ? p[i] : sc_ident<OP>();
        const u64 b = i + 1 < cnt ? p[i + 1] : sc_ident<OP>();
        const u64 s = sc_wave_scan<OP>(sc_comb<OP>(a, b), lane);
        const u64 up = __shfl_up((unsigned long long)s, 1, 64);
        if (lane == 63) s_tot[buf][w] = s;
        __syncthreads();
        u64 pre = run;
#pragma unroll
        for (u32 k = 0; k < 4; ++k) {
            const u64 t = s_tot[buf][k];
            if (k < w) pre = sc_comb<OP>(pre, t);
            run = sc_comb<OP>(run, t);
        }
        const u64 e = sc_comb<OP>(pre, lane ? up : sc_ident<OP>());
        if (i < cnt) p[i] = sc_comb<OP>(init, e);
        if (i + 1 < cnt) p[i + 1] = sc_comb<OP>(init, sc_comb<OP>(e, a));
    }
    if (tid == 0 && total) *total = t9_dec(run, OP, vtype);
}

/* Final combine of the stand-alone fold: one block folds p[0..cnt) and
 * writes the decoded word. */
template <int OP>
__global__ __launch_bounds__(256) void k_fold_top(
    const u64* __restrict__ p, u64 cnt, int vtype, u64* __restrict__ out) {
    __shared__ u64 s_w[4];
    const u32 tid = threadIdx.x;
    u64 acc = sc_ident<OP>();
    for (u64 i = tid; i < cnt; i += 256) acc = sc_comb<OP>(acc, p[i]);
    acc = sc_wave_fold<OP>(acc);
    if ((tid & 63) == 0) s_w[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0)
        *out = t9_dec(sc_comb<OP>(sc_comb<OP>(s_w[0], s_w[1]),
                                  sc_comb<OP>(s_w[2], s_w[3])),
                      OP, vtype);
}

/* n == 0: the operator's decoded identity */
__global__ void k_scan_put(u64* __restrict__ dst, u64 v) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *dst = v;
}

namespace {

bool scan_op_ok(int op, int vtype) {
    if (op < T9_OP_SUM || op > T9_OP_MAX) return false;
    if (vtype < T9_VAL_U64 || vtype > T9_VAL_F64) return false;
    /* a floating sum depends on how the work is split */
    return !(op == T9_OP_SUM && vtype == T9_VAL_F64);
}
u64 ident_enc(int op) { return op == T9_OP_MIN ? ~0ull : 0ull; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

/* T9_SCAN_P1_REVERSE=1: pass 1 visits the tiles in the opposite order to
 * pass 3. Off by default (A/B in DESIGN.md "Scan family"). */
bool p1_reverse() {
    const char* e = getenv("T9_SCAN_P1_REVERSE");
    return e && e[0] == '1';
}

struct ScanWs {
    u64* part;    /* one word per tile */
    u64* part2;   /* one word per T9_SCAN_PART tiles */
    u64 nt, nt2;
};
ScanWs carve(void* ws, u64 n) {
    ScanWs w;
    w.nt = t9_ceil_div(n, T9_SCAN_TILE);
    w.nt2 = t9_ceil_div(w.nt, T9_SCAN_PART);
    w.part = (u64*)ws;
    w.part2 = (u64*)((u8*)ws + t9_align256(w.nt * 8));
    return w;
}

#define T9_SCAN_OP_SWITCH(op, LAUNCH)                                     \
    do {                                                                  \
        if ((op) == T9_OP_SUM) { LAUNCH(T9_OP_SUM); }                     \
        else if ((op) == T9_OP_MIN) { LAUNCH(T9_OP_MIN); }                \
        else { LAUNCH(T9_OP_MAX); }                                       \
    } while (0)

/* pass 2 over w.part[0..nt): exclusive, seeded with `init` (encoded) */
void scan_partials(const ScanWs& w, int op, int vtype, u64 init,
                   u64* d_total, hipStream_t s) {
    if (w.nt <= T9_SCAN_PART) {
#define T9_L(OP)                                                          \
    hipLaunchKernelGGL((k_scan_top<OP>), dim3(1), dim3(256), 0, s, w.part, \
                       w.nt, init, vtype, d_total)
        T9_SCAN_OP_SWITCH(op, T9_L);
#undef T9_L
        return;
    }
    /* the partials are encoded words already: the level below reads them
     * raw (T9_VAL_U64) */
    const u32 g2 = (u32)w.nt2;
    const int pvec = aligned16(w.part);
#define T9_L(OP)                                                          \
    do {                                                                  \
        hipLaunchKernelGGL((k_scan_fold<OP, L_U64, 1>), dim3(g2),         \
                           dim3(256), 0, s, w.part, w.nt, w.nt2,          \
                           (int)T9_VAL_U64, pvec, 0, w.part2);               \
        hipLaunchKernelGGL((k_scan_top<OP>), dim3(1), dim3(256), 0, s,    \
                           w.part2, w.nt2, init, vtype, d_total);         \
        hipLaunchKernelGGL((k_scan_tile<OP, L_U64, 1, 1, true>),          \
                           dim3(g2), dim3(256), 0, s, w.part, w.part,     \
                           w.nt, w.part2, (int)T9_VAL_U64, pvec);            \
    } while (0)
    T9_SCAN_OP_SWITCH(op, T9_L);
#undef T9_L
}

template <int LAYOUT>
int scan_impl(const u64* d_in, u64* d_out, u64 n, int op, int vtype,
              int exclusive, u64 initial, u64* d_total, void* d_workspace,
              hipStream_t s) {
    if (n == 0) {
        if (d_total)
            hipLaunchKernelGGL(k_scan_put, dim3(1), dim3(64), 0, s, d_total,
                               t9_dec(ident_enc(op), op, vtype));
        T9_LAUNCH_CHECK();
        return T9_OK;
    }
    const ScanWs w = carve(d_workspace, n);
    const int vec = aligned16(d_in) && aligned16(d_out);
    const int rev = p1_reverse();
    const u32 g = (u32)w.nt;
    const u64 init = t9_enc(initial, op, vtype);
    constexpr u32 R1 = T9_SCAN_TILE / sc_epr<LAYOUT>();
    constexpr u32 CH = R1 / 8;   /* chunks of 8 rounds: 1 (u64), 2 (pairs) */
    void* tok = t9perf_on() ? t9perf_begin(s, "scan") : nullptr;
#define T9_L(OP)                                                          \
    hipLaunchKernelGGL((k_scan_fold<OP, LAYOUT, R1>), dim3(g), dim3(256),  \
                       0, s, d_in, n, w.nt, vtype, vec, rev, w.part)
    T9_SCAN_OP_SWITCH(op, T9_L);
#undef T9_L
    T9_PERF_WRAP(s, "scan_pass2",
                 scan_partials(w, op, vtype, init, d_total, s));
#define T9_L(OP)                                                          \
    do {                                                                  \
        if (exclusive)                                                    \
            hipLaunchKernelGGL((k_scan_tile<OP, LAYOUT, 8, CH, true>),    \
                               dim3(g), dim3(256), 0, s, d_in, d_out, n,  \
                               w.part, vtype, vec);                       \
        else                                                              \
            hipLaunchKernelGGL((k_scan_tile<OP, LAYOUT, 8, CH, false>),   \
                               dim3(g), dim3(256), 0, s, d_in, d_out, n,  \
                               w.part, vtype, vec);                       \
    } while (0)
    T9_SCAN_OP_SWITCH(op, T9_L);
#undef T9_L
    if (tok) t9perf_end(tok, s);
    T9_LAUNCH_CHECK();
    return T9_OK;
}

} // namespace

extern "C" {

void t9_scan_geometry(uint32_t* tile_elems, uint32_t* partials_per_block) {
    if (tile_elems) *tile_elems = T9_SCAN_TILE;
    if (partials_per_block) *partials_per_block = T9_SCAN_PART;
}

/* one word per tile, one per T9_SCAN_PART tiles, each 256-byte rounded */
u64 t9_scan_workspace(u64 n) {
    const u64 nt = t9_ceil_div(n, T9_SCAN_TILE);
    const u64 nt2 = t9_ceil_div(nt, T9_SCAN_PART);
    return t9_align256(nt * 8) + t9_align256(nt2 * 8) + 256;
}

int t9_scan_u64(t9_context* ctx, const u64* d_in, u64* d_out, u64 n, int op,
                int vtype, int exclusive, u64 initial, u64* d_total,
                void* d_workspace, void* stream) {
    (void)ctx;
    if (!scan_op_ok(op, vtype)) return T9_EINVAL;
    if (exclusive != 0 && exclusive != 1) return T9_EINVAL;
    if (n && (!d_in || !d_out || !d_workspace)) return T9_EINVAL;
    if (t9_ceil_div(n, T9_SCAN_TILE) >= (1ull << 31)) return T9_EINVAL;
    if (n == 0 && !d_total) return T9_OK;
    return scan_impl<L_U64>(d_in, d_out, n, op, vtype, exclusive, initial,
                            d_total, d_workspace, (hipStream_t)stream);
}

int t9_scan_kv(t9_context* ctx, const u8* d_in, u8* d_out, u64 n, int op,
               int vtype, u64 initial, u64* d_total, void* d_workspace,
               void* stream) {
    (void)ctx;
    if (!scan_op_ok(op, vtype)) return T9_EINVAL;
    if (n && (!d_in || !d_out || !d_workspace)) return T9_EINVAL;
    /* pairs are read as u64 words */
    if (((uintptr_t)d_in & 7) || ((uintptr_t)d_out & 7)) return T9_EINVAL;
    if (t9_ceil_div(n, T9_SCAN_TILE) >= (1ull << 31)) return T9_EINVAL;
    if (n == 0 && !d_total) return T9_OK;
    return scan_impl<L_KV>((const u64*)d_in, (u64*)d_out, n, op, vtype, 0,
                           initial, d_total, d_workspace,
                           (hipStream_t)stream);
}

int t9_fold_u64(t9_context* ctx, const u64* d_in, u64 n, u32 stride_words,
                int op, int vtype, u64* d_out, void* d_workspace,
                void* stream) {
    (void)ctx;
    if (!scan_op_ok(op, vtype)) return T9_EINVAL;
    if (stride_words != 1 && stride_words != 2) return T9_EINVAL;
    if (!d_out) return T9_EINVAL;
    if (n && (!d_in || !d_workspace)) return T9_EINVAL;
    const u64 nt = t9_ceil_div(n, T9_SCAN_TILE);
    if (nt >= (1ull << 31)) return T9_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        hipLaunchKernelGGL(k_scan_put, dim3(1), dim3(64), 0, s, d_out,
                           t9_dec(ident_enc(op), op, vtype));
        T9_LAUNCH_CHECK();
        return T9_OK;
    }
    u64* part = (u64*)d_workspace;
    const int vec = aligned16(d_in);
    const u32 g = (u32)(nt < T9_FOLD_GRID ? nt : T9_FOLD_GRID);
    void* tok = t9perf_on() ? t9perf_begin(s, "scan") : nullptr;
#define T9_L(OP)                                                          \
    do {                                                                  \
        if (stride_words == 1)                                            \
            hipLaunchKernelGGL((k_scan_fold<OP, L_U64, 8>), dim3(g),      \
                               dim3(256), 0, s, d_in, n, nt, vtype, vec,  \
                               0, part);                                  \
        else                                                              \
            hipLaunchKernelGGL((k_scan_fold<OP, L_KV, 16>), dim3(g),      \
                               dim3(256), 0, s, d_in, n, nt, vtype, vec,  \
                               0, part);                                  \
        hipLaunchKernelGGL((k_fold_top<OP>), dim3(1), dim3(256), 0, s,    \
                           part, (u64)g, vtype, d_out);                   \
    } while (0)
    T9_SCAN_OP_SWITCH(op, T9_L);
#undef T9_L
    if (tok) t9perf_end(tok, s);
    T9_LAUNCH_CHECK();
    return T9_OK;
}

} /* extern "C" */
