/* thrill_amd.h — C-ABI of libt9.so, the MI355X-native implementation of
 * Thrill's Sort / ReduceByKey DOp hot path (hand-written HIP/CDNA4 kernels,
 * gfx950). This is the drop-in seam of SURVEY.md §8b: the reference's
 * SortNode (thrill/api/sort.hpp:64-787) and ReduceNode
 * (thrill/api/reduce_by_key.hpp:64-239) become thin C++ hosts that marshal
 * item Files <-> device buffers and call these entry points; anything
 * (including a patched reference build) can call the shim directly. The
 * reference-side binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions: all functions are synchronous launches on the passed HIP
 * stream (void* == hipStream_t; NULL = default stream); they return 0 on
 * success or a negative errno-style value. The caller owns every buffer;
 * d_* pointers are device memory. No torch types anywhere.
 *
 * The GPU library contains the PRODUCT path only: it never falls back to
 * CPU. Without a GPU, t9_create fails; nothing here routes through the
 * oracle.
 */
#ifndef THRILL_AMD_H
#define THRILL_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Opaque context: device id, rank, world size, optional RCCL communicator.
 * Mirrors the per-worker api::Context the reference nodes consume
 * (thrill/api/context.hpp:243-245: my_rank / num_workers). */
typedef struct t9_context t9_context;

/* comm: an existing ncclComm_t (RCCL) or NULL for single-GPU use. */
int t9_create(t9_context** out, int device, int rank, int world, void* comm);
int t9_destroy(t9_context* ctx);
const char* t9_version(void);

/* RCCL communicator bootstrap (world > 1): rank 0 generates the unique id
 * (t9_comm_id_size() bytes, = sizeof(ncclUniqueId)), the caller moves it
 * to every rank over any host channel (the reference distributes its TCP
 * endpoints the same way, thrill/api/context.cpp:604-614), then every
 * rank calls t9_comm_init collectively. The context owns the resulting
 * communicator (t9_destroy frees it). Passing an external ncclComm_t via
 * t9_create(comm) remains supported; t9_comm_init on such a context is an
 * error. */
int t9_comm_id_size(void);
int t9_comm_id(void* out_id);
int t9_comm_init(t9_context* ctx, const void* id);

/* ------------------------------------------------------------------ *
 * Synthetic input generation (device-side, seeded; bit-identical to the
 * oracle's t9o_gen_* so CPU/GPU parity runs on identical bytes).
 * Record layout restates examples/terasort/terasort.cpp:31-118.
 * ------------------------------------------------------------------ */
int t9_gen_u64(t9_context* ctx, uint64_t* d_out, uint64_t index0, uint64_t n,
               uint64_t seed, void* stream);
int t9_gen_records(t9_context* ctx, uint8_t* d_out, uint64_t index0,
                   uint64_t n, uint64_t seed, void* stream);

/* ------------------------------------------------------------------ *
 * Local sort — replaces SortAndWriteToFile's std::sort run formation and
 * the loser-tree merge (thrill/api/sort.hpp:665-786,
 * thrill/core/multiway_merge.hpp:30-116): the whole per-GPU partition is
 * sorted in one LSD radix pipeline, so the merge stage vanishes
 * (SURVEY.md §8a row a5/a6).
 * ------------------------------------------------------------------ */

/* Workspace bytes for t9_sort_u64 on n keys. */
uint64_t t9_sort_u64_workspace(uint64_t n);
/* In-place ascending sort of n u64 keys (n < 2^32). */
int t9_sort_u64(t9_context* ctx, uint64_t* d_keys, uint64_t n,
                void* d_workspace, void* stream);

/* Workspace bytes for t9_sort_pairs_u64_u32 on n pairs. */
uint64_t t9_sort_pairs_workspace(uint64_t n);
/* In-place stable ascending sort of (key, payload) pairs by key. */
int t9_sort_pairs_u64_u32(t9_context* ctx, uint64_t* d_keys,
                          uint32_t* d_vals, uint64_t n, void* d_workspace,
                          void* stream);

/* Extract the big-endian u64 prefix of each record's key (bytes
 * key_off .. key_off+7) and the record index iota. rec_size % 4 == 0. */
int t9_extract_key64(t9_context* ctx, const uint8_t* d_recs, uint64_t n,
                     uint32_t rec_size, uint32_t key_off, uint64_t* d_keys,
                     uint32_t* d_idx, void* stream);

/* Little-endian variant: the key is a native uint64_t field (numeric
 * order) — BASELINE config 5's struct{u64 key; u8 payload[120]}. */
int t9_extract_key64_le(t9_context* ctx, const uint8_t* d_recs, uint64_t n,
                        uint32_t rec_size, uint32_t key_off,
                        uint64_t* d_keys, uint32_t* d_idx, void* stream);

/* The fused first pass of the record sort on its own: the u64 key prefix of
 * each record at offset 0 (big-endian, or native little-endian when le != 0),
 * the record index iota unless d_idx is NULL, and d_hist[t * 256 + d] = the
 * number of records of the 8192-record tile t whose top key byte is d
 * (ceil(n / 8192) rows). rec_size is 100 or 128 (T9_EINVAL otherwise);
 * d_recs is 4-byte aligned. */
int t9_extract_key64_hist(t9_context* ctx, const uint8_t* d_recs, uint64_t n,
                          uint32_t rec_size, int le, uint64_t* d_keys,
                          uint32_t* d_idx, uint32_t* d_hist, void* stream);

/* out[i] = recs[idx[i]] for fixed-size records; rec_size is a positive
 * multiple of 4 (T9_EINVAL otherwise, before any device call). */
int t9_gather_records(t9_context* ctx, const uint8_t* d_recs,
                      const uint32_t* d_idx, uint64_t n, uint32_t rec_size,
                      uint8_t* d_out, void* stream);

/* Workspace bytes for t9_sort_records. */
uint64_t t9_sort_records_workspace(uint64_t n, uint32_t rec_size);
/* Sort n fixed-size records by the acceptance total order: lexicographic
 * over the whole record (key prefix first — terasort.cpp:35-37 compares the
 * 10-byte key; ties beyond the radix-sorted u64 key prefix are resolved by
 * comparing the remaining bytes). d_in is preserved; d_out receives the
 * sorted sequence. key_len <= rec_size; key bytes start at offset 0.
 * Equal-u64-prefix runs are re-ordered ON DEVICE (segmented LSD over the
 * tail bytes using the stable pair sort as the primitive; identical
 * chunks are skipped). Synchronizes the stream internally (tie counts
 * and skip flags round-trip to the host). */
int t9_sort_records(t9_context* ctx, const uint8_t* d_in, uint8_t* d_out,
                    uint64_t n, uint32_t rec_size, uint32_t key_len,
                    void* d_workspace, void* stream);

/* config-5 variant: sort records whose key is a native little-endian
 * uint64_t at offset 0 (numeric order; payload-byte tiebreak). */
int t9_sort_records_keyle(t9_context* ctx, const uint8_t* d_in,
                          uint8_t* d_out, uint64_t n, uint32_t rec_size,
                          void* d_workspace, void* stream);

/* How the last t9_sort_records / t9_sort_records_keyle call on ctx was
 * scheduled: 0 = serial (sort everything, then gather), otherwise the
 * number of non-empty chunks whose payload gather ran on the context's
 * internal stream while later sub-buckets were still being sorted (100-byte
 * records on the two-level 9-bit MSB flow with no oversize sub-bucket).
 * The overlapped schedule is OFF by default — measured slower than serial
 * on MI355X — T9_SORT_OVERLAP=1 enables it, =0 forces serial,
 * T9_SORT_OVERLAP_CHUNKS sets the chunk count (default 8, at most 16).
 * The internal stream and its events belong to the
 * context (created on first use, freed by t9_destroy) and are ordered
 * against `stream` by events on both sides, so the call's stream contract
 * is unchanged. A context is driven by ONE host thread at a time. */
int t9_sort_last_schedule(const t9_context* ctx);

/* How the last t9_sort_records / t9_sort_records_keyle call on this context
 * counted keys equal to their neighbour (the probe that decides whether the
 * tie machinery runs): 1 = the sub-bucket sort counted them while it held
 * each sub-bucket sorted (the default two-level flow with every sub-bucket
 * within the single-wave sort's limit); 0 = a standalone pass over the
 * sorted keys (every other flow). The sorted output is the same. */
int t9_sort_last_tiecount(const t9_context* ctx);

/* Whether the last t9_sort_records / t9_sort_records_keyle call on this
 * context ran the fused sub-bucket sort + payload gather kernel (100-byte
 * records on the two-level 9-bit MSB flow, every sub-bucket within 1024
 * records, event timing off, T9_SORT_OVERLAP unset): 1 = it produced the
 * output; 2 = it started, but equal 8-byte prefixes it could not settle in
 * the block made the tie path and a full gather redo the output; 0 = the
 * sort and the gather ran as separate kernels. The fused kernel is the
 * default (measured faster on MI355X);
 * T9_SORT_FUSED_GATHER=0 restores the separate kernels. The sorted output is
 * the same. */
int t9_sort_last_fused(const t9_context* ctx);

/* Whether the last t9_sort_records / t9_sort_records_keyle call on this
 * context ran the packed form of pass 2 and of the fused kernel: one u64 per
 * element, (key bits 46..10) << 27 | record index, used wherever the fused
 * kernel runs and n <= 2^27. 1 = the packed run produced the output; 2 = it
 * started, met a run of more than 8 records whose kept key bits agree, and
 * pass 2 and the fused kernel ran again in the wide form (what
 * t9_sort_last_fused and t9_sort_last_tiecount then report is that wide
 * run); 0 = not used. T9_SORT_PACKED=0 keeps the wide form. The sorted
 * output is the same. */
int t9_sort_last_packed(const t9_context* ctx);

/* ------------------------------------------------------------------ *
 * Classification + partition — replaces TransmitItems' tree-descent loop
 * (thrill/api/sort.hpp:434-535). bucket(item i) = #{ j : (splitter_key[j],
 * splitter_idx[j]) < (key_i, gidx0+i) lexicographically }, which is exactly
 * the tree descent + EqualSampleGreaterIndex walk (sort.hpp:424-426,
 * 487-501) in closed form (proof: oracle/t9_oracle.cpp, cross-checked
 * against the literal tree restatement in tests).
 * ------------------------------------------------------------------ */

/* d_bucket[i] = bucket of key i; d_counts[p] (u64, zeroed by the call)
 * accumulates per-bucket totals. p <= 256. */
int t9_classify_u64(t9_context* ctx, const uint64_t* d_keys, uint64_t n,
                    uint64_t gidx0, const uint64_t* d_spl_keys,
                    const uint64_t* d_spl_idx, uint32_t p,
                    uint32_t* d_bucket, uint64_t* d_counts, void* stream);

/* Record classification under the acceptance total order: primary compare
 * on the precomputed big-endian u64 key prefix (d_k64, from
 * t9_extract_key64), byte fallback over the remaining record bytes on
 * prefix ties, then the splitter-index tiebreak. Splitters are whole
 * records (as in the reference, where splitters are sampled items —
 * api/sort.hpp:300,368-374). */
int t9_classify_rec(t9_context* ctx, const uint8_t* d_recs,
                    const uint64_t* d_k64, uint64_t n, uint64_t gidx0,
                    const uint8_t* d_spl_recs, const uint64_t* d_spl_k64,
                    const uint64_t* d_spl_idx, uint32_t p, uint32_t rec_size,
                    uint32_t* d_bucket, uint64_t* d_counts, void* stream);

/* Workspace bytes for t9_partition_idx. */
uint64_t t9_partition_idx_workspace(uint64_t n);
/* Stable counting-sort of the identity permutation by bucket id:
 * d_perm receives record indices grouped by bucket (bucket-major, original
 * order within a bucket — the scatter of SURVEY.md §8b t9_scatter).
 * d_offsets[p+1] (u64) receives the exclusive bucket start offsets. */
int t9_partition_idx(t9_context* ctx, const uint32_t* d_bucket, uint64_t n,
                     uint32_t p, uint32_t* d_perm, uint64_t* d_offsets,
                     void* d_workspace, void* stream);

/* ------------------------------------------------------------------ *
 * Shuffle — replaces the CatStream/MixStream + Multiplexer TCP exchange
 * (thrill/data/stream_sink.cpp:97-226, multiplexer.cpp:282-463) with an
 * RCCL all-to-all-v over xGMI (grouped ncclSend/ncclRecv), one rank per
 * GPU. counts are element counts per destination rank (host memory);
 * displacements are their exclusive prefix sums (caller-computed).
 * ------------------------------------------------------------------ */
int t9_alltoall(t9_context* ctx, const void* d_send,
                const uint64_t* send_counts, const uint64_t* send_displs,
                void* d_recv, const uint64_t* recv_counts,
                const uint64_t* recv_displs, uint64_t elem_size,
                void* stream);

/* ------------------------------------------------------------------ *
 * Reduce — replaces ReduceProbingHashTable::Insert
 * (thrill/core/reduce_probing_hash_table.hpp:190-268) with a device
 * open-addressing table: linear probing on Hash128to64(salt, key)
 * (thrill/common/hash.hpp:64-72; index mapping
 * core/reduce_functional.hpp:60-72), wave-level pre-combination of equal
 * keys (ballot match + shuffle reduce) before one atomic CAS/ADD per
 * distinct key per wave — the skew control for Zipf keys (SURVEY.md §7
 * step 6). The empty-slot sentinel key 0xFFFF..F is reduced in a dedicated
 * extra slot, mirroring reduce_probing_hash_table.hpp:195-217.
 * Table arrays have capacity+1 entries; capacity must be a power of two
 * >= 2x the number of distinct keys (no grow/spill: 288 GB HBM holds the
 * table — reference grow/spill machinery is subsumed by sizing).
 * ------------------------------------------------------------------ */
/* bucket = Hash128to64(salt, key) % p, the reference's ReduceByHash
 * partition mapping (core/reduce_functional.hpp:60-72; libstdc++
 * std::hash<u64> is the identity) — splits pre-reduced pairs across ranks.
 * d_counts[p] (u64, zeroed by the call) accumulates per-rank totals. */
int t9_hash_bucket(t9_context* ctx, const uint64_t* d_keys, uint64_t n,
                   uint64_t salt, uint32_t p, uint32_t* d_bucket,
                   uint64_t* d_counts, void* stream);

/* The reduce table is ONE interleaved u64 array of 2*(capacity+1)
 * elements: slot i = (d_table[2i] key, d_table[2i+1] sum), aux sentinel
 * slot at [2*capacity .. 2*capacity+1]. Interleaving keeps each probing
 * CAS + add inside one cache line (the build of a big-vocab stream is
 * random-line bound). capacity must be a power of two. */
int t9_reduce_init(t9_context* ctx, uint64_t* d_table, uint64_t capacity,
                   void* stream);
/* Accumulate n (key, value) pairs into the table; value reduce = u64 add.
 * d_error (device u32, zeroed by the call) is set nonzero if the table
 * overflows. */
int t9_reduce_build(t9_context* ctx, const uint64_t* d_keys,
                    const uint64_t* d_vals, uint64_t n,
                    uint64_t* d_table, uint64_t capacity, uint64_t salt,
                    uint32_t* d_error, void* stream);
/* Compact occupied slots to (key, value) arrays (unordered);
 * d_out_n (device u64) receives the count. */
int t9_reduce_drain(t9_context* ctx, const uint64_t* d_table,
                    uint64_t capacity, uint64_t* d_out_keys,
                    uint64_t* d_out_vals, uint64_t* d_out_n, void* stream);

/* ------------------------------------------------------------------ *
 * 128-bit composite-key reduce — config-4 string identity. The
 * reference reduces (std::string, u64) with equality on the FULL key
 * (core/reduce_probing_hash_table.hpp:233); here words are
 * dictionary-encoded at tokenize time into TWO independent 64-bit
 * hashes (k1, k2) and reduced on the 128-bit composite: distinct words
 * stay separate unless both hashes collide (p ~= 2^-128 per pair; a
 * forced k1 collision stays separate — parity-tested). Table slot = 3
 * interleaved u64 {k1, k2, sum}, 3*capacity array, capacity a power of
 * two. k1 == ~0 / k2 == ~0 are reserved sentinels (t9_hash2_of remaps
 * them). d_vals == NULL means every pair counts 1.
 *
 * Knobs of the plain path, read from the environment on every call:
 * T9_LDS128_SLOTS picks the per-block LDS filter (>= 4096: 4096, the
 * default; <= 1024: 1024; otherwise 2048), T9_R128_READFIRST=0 turns the
 * read-before-CAS probing off (the 1024 filter always runs without it),
 * T9_REDUCE_GRID fixes the build grid, and T9_R128_STRIDE=4 pads every
 * slot to 4 u64 {k1, k2, sum, unused}: init, build, drain and lookup then
 * all address a 4*capacity array. Allocate t9_reduce128_table_words
 * (capacity) u64 — 3*capacity, or 4*capacity under that knob — not a
 * literal 3*capacity. The 4-word stride is built for the (4096,
 * read-first) variant only: with T9_R128_STRIDE=4 and T9_R128_READFIRST=0
 * or T9_LDS128_SLOTS < 4096, t9_reduce128_build returns T9_EINVAL before
 * any device call — never a mixed layout.
 * ------------------------------------------------------------------ */
/* u64 elements of a 128-bit table of `capacity` slots under the current
 * T9_R128_STRIDE; pure host code. */
uint64_t t9_reduce128_table_words(uint64_t capacity);
int t9_reduce128_init(t9_context* ctx, uint64_t* d_table,
                      uint64_t capacity, void* stream);
int t9_reduce128_build(t9_context* ctx, const uint64_t* d_k1,
                       const uint64_t* d_k2, const uint64_t* d_vals,
                       uint64_t n, uint64_t* d_table, uint64_t capacity,
                       uint64_t salt, uint32_t* d_error, void* stream);
int t9_reduce128_drain(t9_context* ctx, const uint64_t* d_table,
                       uint64_t capacity, uint64_t* d_out_k1,
                       uint64_t* d_out_k2, uint64_t* d_out_vals,
                       uint64_t* d_out_n, void* stream);
/* Read-only probe of a built 128-bit table: d_slot[i] = slot index holding
 * (k1[i], k2[i]), or 0xFFFFFFFF if absent. capacity <= 2^31. Same start
 * slot, probe order and slot stride as build/init/drain; at most
 * `capacity` probes per key, so a full table terminates. Slot indices give
 * every reduced group a dense-enough integer name (< capacity) without a
 * host-side decode map. */
int t9_reduce128_lookup(t9_context* ctx, const uint64_t* d_k1,
                        const uint64_t* d_k2, uint64_t n,
                        const uint64_t* d_table, uint64_t capacity,
                        uint64_t salt, uint32_t* d_slot, void* stream);
/* two independent 64-bit hashes of u64 token ids (synthetic stand-in for
 * hashing the word bytes at tokenize time; remaps the reserved
 * sentinels) */
int t9_hash2_of(t9_context* ctx, const uint64_t* d_ids, uint64_t n,
                uint64_t* d_k1, uint64_t* d_k2, void* stream);
/* bucket = key % p — the partition mapping when the key already is the
 * hash (128-bit path partitions on k1, mirroring h % num_partitions,
 * core/reduce_functional.hpp:60-72) */
int t9_bucket_mod(t9_context* ctx, const uint64_t* d_keys, uint64_t n,
                  uint32_t p, uint32_t* d_bucket, uint64_t* d_counts,
                  void* stream);

/* ------------------------------------------------------------------ *
 * Real text — the word_count PreOp on the device. ReadLines splits at
 * '\n' (thrill/api/read_lines.hpp) and WordCount splits lines at ' ',
 * dropping empty words (examples/word_count/word_count.hpp:37-45): a
 * token is a maximal run of bytes that are neither 0x20 nor 0x0A. Every
 * other byte value (0x00, '\t', '\r', 0x80-0xFF) is a word byte, and a
 * token running to the end of the buffer is a token. Together with
 * t9_reduce128_* and t9_reduce128_lookup these give (word, count) pairs
 * from raw bytes with 128-bit identity end to end (DESIGN.md "Real text:
 * device tokenizer and hasher").
 * ------------------------------------------------------------------ */

/* Workspace bytes for t9_text_tokenize; pure host code. */
uint64_t t9_text_tokenize_workspace(uint64_t nbytes);
/* Tokens of d_text[0..nbytes) in text order. d_text 16-byte aligned,
 * nbytes < 2^32 (T9_EINVAL otherwise). d_tok_off[i] = byte offset of
 * token i, d_tok_len[i] = its length (>= 1), *d_ntok (device u64, zeroed
 * by the call) = count. d_tok_off == NULL && d_tok_len == NULL: count
 * only. Output capacity (nbytes+1)/2 always suffices. Never touches a
 * byte outside [d_text, d_text+nbytes). */
int t9_text_tokenize(t9_context* ctx, const uint8_t* d_text,
                     uint64_t nbytes, uint32_t* d_tok_off,
                     uint32_t* d_tok_len, uint64_t* d_ntok,
                     void* d_workspace, void* stream);

/* (k1, k2) of n byte ranges of d_text (8-byte aligned): FNV-1a over the
 * unsigned bytes under two bases, each mixed by Hash128to64, reserved
 * sentinels remapped — bit-equal to detail::string_hash2 of t9/dia.hpp.
 * len 0 is legal (hash of the empty string). Never reads outside
 * [d_text, d_text+nbytes); off+len > nbytes for any i is a caller error
 * reported through d_error (device u32, zeroed by the call), not a read
 * (that entry's k1/k2 are written as 0). */
int t9_text_hash2(t9_context* ctx, const uint8_t* d_text, uint64_t nbytes,
                  const uint32_t* d_off, const uint32_t* d_len, uint64_t n,
                  uint64_t* d_k1, uint64_t* d_k2, uint32_t* d_error,
                  void* stream);

/* d_first[s] = min{ i : d_slot[i] == s }, 0xFFFFFFFF for untouched slots;
 * d_first has `capacity` entries and is initialised by the call.
 * n < 2^32. Entries of d_slot equal to 0xFFFFFFFF (or >= capacity) are
 * skipped. With d_slot from t9_reduce128_lookup over all tokens this
 * names each group's first occurrence — the spelling to report. */
int t9_text_first_token(t9_context* ctx, const uint32_t* d_slot, uint64_t n,
                        uint32_t* d_first, uint64_t capacity, void* stream);

/* ReduceToIndex — reference
 * api/reduce_to_index.hpp + core/reduce_by_index_post_phase.hpp with the
 * ReduceByIndex mapping (core/reduce_functional.hpp:84-149): keys are
 * dense indices in [begin, begin+size); d_dense (size u64, zeroed by the
 * call) accumulates the per-index sums; absent indices stay at the
 * neutral 0, as the reference's by-index post phase emits. d_error set
 * nonzero on out-of-range keys. */
int t9_reduce_by_index(t9_context* ctx, const uint64_t* d_keys,
                       const uint64_t* d_vals, uint64_t n, uint64_t begin,
                       uint64_t size, uint64_t* d_dense, uint32_t* d_error,
                       void* stream);

/* by-index partition: bucket = (key-begin)*p/size
 * (core/reduce_functional.hpp:113-128). Out-of-range keys clamp to the
 * last partition and set d_error (same error model as
 * t9_reduce_by_index). */
int t9_index_bucket(t9_context* ctx, const uint64_t* d_keys, uint64_t n,
                    uint64_t begin, uint64_t size, uint32_t p,
                    uint32_t* d_bucket, uint64_t* d_counts,
                    uint32_t* d_error, void* stream);

/* ------------------------------------------------------------------ *
 * Reduce operators — the three tables above with a selectable reduce
 * function. The reference's reduce_function is any associative
 * (V, V) -> V (core/reduce_probing_hash_table.hpp:233); the operators
 * with a native 64-bit atomic run here: SUM, MIN, MAX, over values read
 * as u64, i64 (two's-complement order) or f64. F64 order is the IEEE-754
 * totalOrder of the bit patterns: -NaN < -inf < ... < -0.0 < +0.0 < ...
 * < +inf < +NaN — total and deterministic, so results are bit-exact
 * however the atomics interleave. SUM is the wrapping 64-bit add (the
 * same for U64 and I64); SUM with F64 is T9_EINVAL, because a floating
 * atomic sum depends on arrival order (DESIGN.md "Reduce operators").
 *
 * Each _op function takes the parameters of the function it parallels
 * plus (op, vtype). Layouts, capacity rules, the sentinel-key aux slot,
 * probe order, salt, the error model and the stream contract are
 * unchanged, so t9_reduce128_lookup works on a table built with any
 * operator. What differs is the value word: init_op fills it with the
 * operator's identity (0 for SUM, all-ones for MIN, 0 for MAX), and for
 * MIN and MAX the table holds ENCODED values — I64: bits ^ 1<<63; F64:
 * bits ^ (sign ? ~0 : 1<<63) — which order as unsigned integers;
 * drain_op decodes. A table carries no operator tag: init_op, build_op
 * and drain_op must be called with the same (op, vtype); mixing them, or
 * mixing _op calls with the plain ones on one table, is a caller error.
 *
 * Every _op function validates op, vtype, pointers and the power-of-two
 * capacity before any device call. The operator path instantiates fewer
 * kernel variants than the plain one: T9_LDS_SLOTS / T9_LDS128_SLOTS
 * select 1024 (<= 1024) or 4096 slots, T9_REDUCE_GRID,
 * T9_REDUCE_READFIRST and T9_R128_READFIRST are honoured,
 * T9_REDUCE_COMBINE and T9_REDUCE_WAVECOMB are served by the LDS variant
 * (same layout, same result), and T9_R128_STRIDE=4 is refused with
 * T9_EINVAL by every t9_reduce128_*_op call.
 * ------------------------------------------------------------------ */
typedef enum { T9_OP_SUM = 0, T9_OP_MIN = 1, T9_OP_MAX = 2 } t9_reduce_op;
typedef enum { T9_VAL_U64 = 0, T9_VAL_I64 = 1, T9_VAL_F64 = 2 } t9_val_type;

/* op / vtype are passed as int so that an out-of-range value is a
 * T9_EINVAL, not undefined behaviour. Values travel as their 64-bit
 * patterns in uint64_t arrays whatever vtype says. */
int t9_reduce_init_op(t9_context* ctx, uint64_t* d_table, uint64_t capacity,
                      int op, int vtype, void* stream);
int t9_reduce_build_op(t9_context* ctx, const uint64_t* d_keys,
                       const uint64_t* d_vals, uint64_t n,
                       uint64_t* d_table, uint64_t capacity, uint64_t salt,
                       int op, int vtype, uint32_t* d_error, void* stream);
int t9_reduce_drain_op(t9_context* ctx, const uint64_t* d_table,
                       uint64_t capacity, int op, int vtype,
                       uint64_t* d_out_keys, uint64_t* d_out_vals,
                       uint64_t* d_out_n, void* stream);

/* d_vals == NULL ("every pair counts 1") is valid only with T9_OP_SUM;
 * T9_EINVAL otherwise. */
int t9_reduce128_init_op(t9_context* ctx, uint64_t* d_table,
                         uint64_t capacity, int op, int vtype,
                         void* stream);
int t9_reduce128_build_op(t9_context* ctx, const uint64_t* d_k1,
                          const uint64_t* d_k2, const uint64_t* d_vals,
                          uint64_t n, uint64_t* d_table, uint64_t capacity,
                          uint64_t salt, int op, int vtype,
                          uint32_t* d_error, void* stream);
int t9_reduce128_drain_op(t9_context* ctx, const uint64_t* d_table,
                          uint64_t capacity, int op, int vtype,
                          uint64_t* d_out_k1, uint64_t* d_out_k2,
                          uint64_t* d_out_vals, uint64_t* d_out_n,
                          void* stream);

/* ReduceToIndex with an operator and a neutral element (reference
 * api/dia.hpp:1346-1351): d_dense[i] is the fold of the values whose key
 * is begin + i, or `neutral` if NO item has that key. The neutral element
 * is not folded in (core/reduce_by_index_post_phase.hpp:150-172), and an
 * index whose only values equal the operator's identity still yields that
 * value: "untouched" is recorded in a bitmap in d_workspace
 * (t9_reduce_by_index_op_workspace(size) bytes; pure host code).
 * Out-of-range keys set d_error, as in t9_reduce_by_index. */
uint64_t t9_reduce_by_index_op_workspace(uint64_t size);
int t9_reduce_by_index_op(t9_context* ctx, const uint64_t* d_keys,
                          const uint64_t* d_vals, uint64_t n,
                          uint64_t begin, uint64_t size, int op, int vtype,
                          uint64_t neutral, uint64_t* d_dense,
                          uint32_t* d_error, void* d_workspace,
                          void* stream);

/* ------------------------------------------------------------------ *
 * Scan family — PrefixSum / ExPrefixSum and the fold behind the Sum / Min
 * / Max actions (reference api/prefix_sum.hpp:92-110, api/all_reduce.hpp)
 * with the operators and value types of "Reduce operators" above. With ⊕
 * the operator and `initial` a 64-bit pattern read as vtype:
 *   inclusive: out[i] = initial ⊕ x[0] ⊕ … ⊕ x[i]
 *   exclusive: out[0] = initial, out[i] = initial ⊕ x[0] ⊕ … ⊕ x[i-1]
 * SUM is the wrapping 64-bit add (the same for U64 and I64); MIN and MAX
 * order values as unsigned, two's-complement or IEEE-754 totalOrder; SUM
 * with F64 is T9_EINVAL. Every result is bit-exact and does not depend on
 * how the work is split (DESIGN.md "Scan family").
 *
 * A scan is three launches on `stream` — fold every tile, scan the tile
 * totals, scan every tile from its carry — and no block waits on another.
 * t9_scan_geometry reports the tile size in elements and how many tile
 * totals one block of the middle pass covers (above that count a second
 * level runs); pure host code. t9_scan_workspace(n) bytes of d_workspace
 * serve t9_scan_u64, t9_scan_kv and t9_fold_u64 on n elements; pure host
 * code. The workspace need not be zeroed, nothing in it survives a call,
 * and it should be 16-byte aligned (hipMalloc memory is).
 *
 * d_out == d_in (in place) is allowed; otherwise d_in is not written.
 * Pointers aligned to 16 bytes get 16-byte accesses; 8-byte alignment is
 * enough for correctness. If d_total is non-NULL it receives the fold of
 * the n inputs WITHOUT `initial`.
 *
 * t9_scan_kv scans 16-byte {u64 key, 64-bit value} pairs, inclusive only:
 * the key is copied through and the value word is scanned — the
 * PrefixSum([](a, b){ return { b.key, op(a.value, b.value) }; }) idiom of
 * examples/suffix_sorting/prefix_doubling.cpp:346-351; `initial` seeds the
 * value word. An exclusive scan over pairs would shift the keys and is not
 * offered.
 *
 * t9_fold_u64 folds n values read every stride_words u64 words (1 =
 * contiguous, 2 = the value word of n pairs: pass the address of the
 * first pair) into *d_out (device u64).
 *
 * Validation comes before any device call; each of these is T9_EINVAL:
 * op or vtype out of range, SUM with F64, exclusive not 0 or 1,
 * stride_words not 1 or 2, a NULL in, out or workspace pointer with
 * n > 0, NULL d_out of the fold, 2^31 tiles or more. With n == 0, d_total
 * and the fold's d_out receive the operator's identity as a value of
 * vtype: 0 for SUM; for MIN the top of the order (all-ones, INT64_MAX,
 * the largest +NaN); for MAX the bottom (0, INT64_MIN, the largest -NaN).
 * With n == 0 and d_total == NULL a scan returns T9_OK without touching
 * the device.
 * ------------------------------------------------------------------ */
void t9_scan_geometry(uint32_t* tile_elems, uint32_t* partials_per_block);
uint64_t t9_scan_workspace(uint64_t n);
int t9_scan_u64(t9_context* ctx, const uint64_t* d_in, uint64_t* d_out,
                uint64_t n, int op, int vtype, int exclusive,
                uint64_t initial, uint64_t* d_total, void* d_workspace,
                void* stream);
int t9_scan_kv(t9_context* ctx, const uint8_t* d_in, uint8_t* d_out,
               uint64_t n, int op, int vtype, uint64_t initial,
               uint64_t* d_total, void* d_workspace, void* stream);
int t9_fold_u64(t9_context* ctx, const uint64_t* d_in, uint64_t n,
                uint32_t stride_words, int op, int vtype, uint64_t* d_out,
                void* d_workspace, void* stream);

/* ------------------------------------------------------------------ *
 * InnerJoin — the matching half of the reference's sort-based join
 * (thrill/api/inner_join.hpp:213-287): the list of all index pairs (i, j)
 * with lkeys[i] == rkeys[j], ordered by key ascending as unsigned 64-bit,
 * then by i ascending, then by j ascending. Every u64 value is a legal key
 * (no sentinel); the inputs are not modified; the result is a deterministic
 * function of the inputs (no atomics, no hash table). Payloads are not the
 * join's business: materialise rows with t9_gather_records on the two
 * index arrays.
 *
 * t9_join_count sorts (key, index) pairs of both sides stably, finds every
 * left element's range of equal right keys, scans the range lengths, leaves
 * all of that in d_workspace, synchronises the stream and returns the
 * number of result pairs through the HOST pointer `total` (one word read
 * back). t9_join_emit writes positions [0, min(n_out, total)) of the result
 * and touches nothing else: a short buffer receives a prefix. It needs the
 * n_left / n_right / d_workspace of the count, launches on `stream` without
 * synchronising, and may be called more than once on one workspace. Work is
 * divided by output position, so one key that is hot on both sides costs
 * per row what unique keys cost (DESIGN.md "Join").
 *
 * t9_join_geometry: left keys per block of the matching kernel, output
 * positions per block of the emit kernel, and the most right keys a matching
 * block stages in LDS (a longer candidate slice is searched in global
 * memory). t9_join_workspace(n_left, n_right) bytes, monotone in both,
 * include the nested sort and scan workspaces; d_workspace must be 16-byte
 * aligned (hipMalloc memory is) and need not be zeroed. Both are pure host
 * code. Two A/B knobs, read on every call, change speed only:
 * T9_JOIN_GALLOP=0 (plain binary search for the upper bound) and
 * T9_JOIN_EMIT_V4=0 (4-byte instead of 16-byte stores; also what runs when
 * an output pointer is not 16-byte aligned).
 *
 * Validation comes before any device call; each of these is T9_EINVAL:
 * n_left or n_right >= 2^32, NULL total, NULL keys of a non-empty side,
 * NULL or misaligned d_workspace, a NULL output with n_out > 0, 2^31 output
 * tiles or more. An empty side gives *total = 0 and T9_OK without a launch
 * (the reference returns early there too), and t9_join_emit with an empty
 * side or n_out == 0 is T9_OK without a launch.
 * ------------------------------------------------------------------ */
void t9_join_geometry(uint32_t* left_tile, uint32_t* out_tile,
                      uint32_t* stage_keys);
uint64_t t9_join_workspace(uint64_t n_left, uint64_t n_right);
int t9_join_count(t9_context* ctx, const uint64_t* d_lkeys, uint64_t n_left,
                  const uint64_t* d_rkeys, uint64_t n_right,
                  uint64_t* total, void* d_workspace, void* stream);
int t9_join_emit(t9_context* ctx, uint64_t n_left, uint64_t n_right,
                 const void* d_workspace, uint64_t n_out,
                 uint32_t* d_out_left, uint32_t* d_out_right, void* stream);

/* GroupByKey support (SURVEY.md §8f item 3 — thrill/api/group_by_key.hpp
 * is sort-based): the group index of a key-sorted array. d_unique[g] /
 * d_offsets[g] (ascending run starts) for g in [0, *d_count); d_count is
 * a device u64. Output capacity n always suffices. */
uint64_t t9_group_index_workspace(uint64_t n);
int t9_group_index(t9_context* ctx, const uint64_t* d_sorted_keys,
                   uint64_t n, uint64_t* d_unique, uint64_t* d_offsets,
                   uint64_t* d_count, void* d_workspace, void* stream);

/* Merge two byte-lexicographically sorted fixed-size record sequences
 * (the reference Merge's comparator restricted to the GPU-executable
 * byte order, api/merge.hpp:368-520); equal records from d_a precede
 * those from d_b. rec_size % 4 == 0. */
int t9_merge_records(t9_context* ctx, const uint8_t* d_a, uint64_t na,
                     const uint8_t* d_b, uint64_t nb, uint32_t rec_size,
                     uint8_t* d_out, void* stream);

/* Merge (SURVEY.md §8f item 4 — thrill/api/merge.hpp merges pre-sorted
 * DIAs): merge two sorted u64 sequences into d_out (na+nb); equal keys
 * from d_a precede those from d_b. One merge-path pass. */
int t9_merge_u64(t9_context* ctx, const uint64_t* d_a, uint64_t na,
                 const uint64_t* d_b, uint64_t nb, uint64_t* d_out,
                 void* stream);

/* Zipf(s, q, N) token sampling by inverse CDF (bit-identical to the
 * oracle's t9o_zipf_tokens given the same d_cdf table — the CDF itself is
 * computed once by the oracle/host and copied to the device). Restates
 * thrill/common/zipf_distribution.hpp:55-120's mass function. */
int t9_zipf_tokens(t9_context* ctx, uint64_t* d_out, const double* d_cdf,
                   uint64_t N, uint64_t index0, uint64_t n, uint64_t seed,
                   void* stream);

/* ------------------------------------------------------------------ *
 * Optional per-kernel-class HIP event timing (off by default) for the
 * bench harness's roofline measurement. Classes: "pair_scatter",
 * "keys_scatter", "hist_pairs", "hist_keys", "extract", "gather",
 * "reduce_build_op", "scan" (one t9_scan_* or t9_fold_u64 call, all its
 * launches), "scan_pass2" (the middle pass of a scan alone), "join_bounds"
 * and "join_emit" (the two kernels of t9_join_count / t9_join_emit).
 * ------------------------------------------------------------------ */
int t9_perf_enable(int on);
int t9_perf_read(const char* kernel_class, double* total_ms,
                 uint64_t* launches);
int t9_perf_reset(void);

#ifdef __cplusplus
}
#endif

#endif /* THRILL_AMD_H */
