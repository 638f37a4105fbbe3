/* t9/dia.hpp — C++ operator surface mirroring the reference's DIA API for
 * the Sort/ReduceByKey hot path, executing on the GPU through the C ABI of
 * thrill_amd.h. Names, argument meaning and error behaviour follow
 * thrill/api/dia.hpp (Sort :798-937, ReduceByKey via ReducePair
 * :241-463, Generate api/generate.hpp:37, Size api/size.hpp:28,
 * AllGather api/all_gather.hpp) restricted to the GPU-executable contract:
 * fixed-size POD items, byte-lexicographic (or u64) key order, 64-bit
 * sum / min / max reduction. There is NO CPU execution path here — without a GPU,
 * Context construction fails (the CPU restatement lives in oracle/ and is
 * test infrastructure).
 *
 * Execution model: eager per-op evaluation (each DOp runs when
 * constructed) on a single rank; the reference's lazy Stage/Execute
 * machinery (api/dia_base.cpp:381-443) is unnecessary for the two target
 * pipelines, whose DAGs are straight lines — see DESIGN.md. Multi-rank
 * execution goes through the python pipeline (thrill_amd/pipeline.py) or
 * the C ABI's own RCCL bootstrap (t9_comm_id/t9_comm_init).
 *
 * Round 2 additions, driven by the verbatim example ports (examples/):
 * host-side DIAs for non-POD items (std::string lines), FlatMap, and a
 * generic ReduceByKey for (string, u64-counter) pairs that
 * dictionary-encodes words and reduces on the GPU 128-bit composite
 * table (string identity — DESIGN.md "Config-4 string identity").
 *
 * TextWordCount takes raw text bytes instead: tokenizing, hashing,
 * reducing and choosing one spelling per word all run on the device
 * (DESIGN.md "Real text: device tokenizer and hasher").
 *
 * PrefixSum / ExPrefixSum and the Sum / Min / Max / AllReduce actions run
 * on the device (t9_scan_u64 / t9_scan_kv / t9_fold_u64) for a probed +,
 * min or max over 64-bit scalar items and for the { b.key, op(a.value,
 * b.value) } shape over KeyValue; everything else folds on the host in the
 * reference's own order (DESIGN.md "Scan family").
 *
 * InnerJoin matches the extracted keys of two DIAs on the device
 * (t9_join_count / t9_join_emit) and applies the join function on the host
 * to the index pairs that come back (DESIGN.md "Join").
 */
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../thrill_amd.h"

#include <fcntl.h>
#include <unistd.h>

namespace t9 {
namespace api {

namespace detail {

//! O_DIRECT bulk file write through a 16 MiB aligned bounce buffer —
//! the buffered+fsync path measured 1.8 GB/s against the box medium's
//! 8.2 GB/s O_DIRECT line rate (profiles/r02_io_bench.json notes); the
//! unaligned tail goes through a buffered descriptor. Falls back to
//! stdio wholesale if O_DIRECT open fails (filesystem-dependent).
inline bool write_file_direct(const char* name, const void* data,
                              size_t bytes) {
    const size_t CH = 16u << 20, ALIGN = 4096;
    int fd = ::open(name, O_WRONLY | O_CREAT | O_TRUNC | O_DIRECT, 0644);
    if (fd < 0) return false;
    void* buf = nullptr;
    if (posix_memalign(&buf, ALIGN, CH) != 0) {
        ::close(fd);
        return false;
    }
    const size_t aligned = bytes / ALIGN * ALIGN;
    size_t off = 0;
    bool ok = true;
    while (ok && off < aligned) {
        size_t len = std::min(CH, aligned - off);
        std::memcpy(buf, (const char*)data + off, len);
        ok = ::write(fd, buf, len) == (ssize_t)len;
        off += len;
    }
    ::fsync(fd);
    ::close(fd);
    std::free(buf);
    if (ok && aligned < bytes) {
        int fd2 = ::open(name, O_WRONLY);
        ok = fd2 >= 0 &&
             ::pwrite(fd2, (const char*)data + aligned, bytes - aligned,
                      (off_t)aligned) == (ssize_t)(bytes - aligned);
        if (fd2 >= 0) {
            ::fsync(fd2);
            ::close(fd2);
        }
    }
    return ok;
}

inline bool read_file_direct(const char* name, void* data, size_t bytes) {
    const size_t CH = 16u << 20, ALIGN = 4096;
    int fd = ::open(name, O_RDONLY | O_DIRECT);
    if (fd < 0) return false;
    void* buf = nullptr;
    if (posix_memalign(&buf, ALIGN, CH) != 0) {
        ::close(fd);
        return false;
    }
    const size_t aligned = bytes / ALIGN * ALIGN;
    size_t off = 0;
    bool ok = true;
    while (ok && off < aligned) {
        size_t len = std::min(CH, aligned - off);
        ok = ::read(fd, buf, len) == (ssize_t)len;
        if (ok) std::memcpy((char*)data + off, buf, len);
        off += len;
    }
    ::close(fd);
    std::free(buf);
    if (ok && aligned < bytes) {
        int fd2 = ::open(name, O_RDONLY);
        ok = fd2 >= 0 &&
             ::pread(fd2, (char*)data + aligned, bytes - aligned,
                     (off_t)aligned) == (ssize_t)(bytes - aligned);
        if (fd2 >= 0) ::close(fd2);
    }
    return ok;
}

//! device-buffer -> file, O_DIRECT, PINNED ping-pong staging: the
//! pageable AllGather D2H measured ~1.5-2 GB/s and throttled the whole
//! write; pinned transfers overlap the previous chunk's disk write.
//! Returns false to signal the caller's fallback.
inline bool write_device_direct(const char* name, const void* d_ptr,
                                size_t bytes, hipStream_t s) {
    const size_t CH = 64u << 20;   /* 64 MiB: fewer sync/chunk overheads */
    int fd = ::open(name, O_WRONLY | O_CREAT | O_TRUNC | O_DIRECT, 0644);
    if (fd < 0) return false;
    void* pin[2] = { nullptr, nullptr };
    void* dbuf = nullptr;   /* plain aligned bounce: O_DIRECT DMA from
                               GPU-registered pinned pages measured
                               ~3x slower than from normal memory */
    if (hipHostMalloc(&pin[0], CH, 0) != hipSuccess ||
        hipHostMalloc(&pin[1], CH, 0) != hipSuccess ||
        posix_memalign(&dbuf, 4096, CH) != 0) {
        if (pin[0]) (void)hipHostFree(pin[0]);
        if (pin[1]) (void)hipHostFree(pin[1]);
        ::close(fd);
        return false;
    }
    const size_t ALIGN = 4096;
    const size_t aligned = bytes / ALIGN * ALIGN;
    bool ok = true;
    size_t off = 0;
    int cur = 0;
    size_t len0 = std::min(CH, aligned);
    if (len0)
        ok = hipMemcpyAsync(pin[0], (const char*)d_ptr, len0,
                            hipMemcpyDeviceToHost, s) == hipSuccess;
    while (ok && off < aligned) {
        const size_t len = std::min(CH, aligned - off);
        ok = hipStreamSynchronize(s) == hipSuccess;
        const size_t noff = off + len;
        if (ok && noff < aligned) {
            const size_t nlen = std::min(CH, aligned - noff);
            ok = hipMemcpyAsync(pin[cur ^ 1], (const char*)d_ptr + noff,
                                nlen, hipMemcpyDeviceToHost,
                                s) == hipSuccess;
        }
        /* write straight from the pinned buffer: an A/B with a plain
         * aligned bounce measured WORSE on the write side (box-variable
         * storage; profiles/r02_io_bench.json notes) */
        ok = ok && ::write(fd, pin[cur], len) == (ssize_t)len;
        off = noff;
        cur ^= 1;
    }
    std::free(dbuf);
    (void)dbuf;
    ::fsync(fd);
    ::close(fd);
    if (ok && aligned < bytes) {
        ok = hipMemcpy(pin[0], (const char*)d_ptr + aligned,
                       bytes - aligned, hipMemcpyDeviceToHost) ==
             hipSuccess;
        int fd2 = ::open(name, O_WRONLY);
        ok = ok && fd2 >= 0 &&
             ::pwrite(fd2, pin[0], bytes - aligned, (off_t)aligned) ==
                 (ssize_t)(bytes - aligned);
        if (fd2 >= 0) {
            ::fsync(fd2);
            ::close(fd2);
        }
    }
    (void)hipHostFree(pin[0]);
    (void)hipHostFree(pin[1]);
    return ok;
}

//! file -> device buffer, O_DIRECT, pinned ping-pong (mirror of the
//! writer: disk read of chunk i overlaps the H2D copy of chunk i-1)
inline bool read_device_direct(const char* name, void* d_ptr,
                               size_t bytes, hipStream_t s) {
    const size_t CH = 64u << 20;
    int fd = ::open(name, O_RDONLY | O_DIRECT);
    if (fd < 0) return false;
    void* pin[2] = { nullptr, nullptr };
    if (hipHostMalloc(&pin[0], CH, 0) != hipSuccess ||
        hipHostMalloc(&pin[1], CH, 0) != hipSuccess) {
        if (pin[0]) (void)hipHostFree(pin[0]);
        ::close(fd);
        return false;
    }
    const size_t ALIGN = 4096;
    const size_t aligned = bytes / ALIGN * ALIGN;
    bool ok = true;
    size_t off = 0;
    int cur = 0;
    void* dbuf2 = nullptr;
    if (posix_memalign(&dbuf2, ALIGN, CH) != 0) {
        (void)hipHostFree(pin[0]);
        (void)hipHostFree(pin[1]);
        ::close(fd);
        return false;
    }
    while (ok && off < aligned) {
        const size_t len = std::min(CH, aligned - off);
        /* O_DIRECT into plain aligned memory, then host->pinned, then
         * async H2D; the disk read of the next chunk overlaps the H2D
         * (sync only before reusing the pinned buffer) */
        ok = ::read(fd, dbuf2, len) == (ssize_t)len;
        if (ok) {
            std::memcpy(pin[cur], dbuf2, len);
            ok = hipMemcpyAsync((char*)d_ptr + off, pin[cur], len,
                                hipMemcpyHostToDevice, s) == hipSuccess;
        }
        cur ^= 1;
        off += len;
        /* sync unconditionally: the tail path below reuses pin[0], and
         * the next iteration reuses the flipped buffer — either way the
         * in-flight H2D must drain first (an intermittent corruption of
         * the LAST chunk escaped when this sync was skipped on the
         * final iteration) */
        if (ok)
            ok = hipStreamSynchronize(s) == hipSuccess;
    }
    std::free(dbuf2);
    ::close(fd);
    if (ok && aligned < bytes) {
        int fd2 = ::open(name, O_RDONLY);
        ok = fd2 >= 0 &&
             ::pread(fd2, pin[0], bytes - aligned, (off_t)aligned) ==
                 (ssize_t)(bytes - aligned);
        if (fd2 >= 0) ::close(fd2);
        if (ok)
            ok = hipMemcpyAsync((char*)d_ptr + aligned, pin[0],
                                bytes - aligned, hipMemcpyHostToDevice,
                                s) == hipSuccess;
    }
    ok = ok && hipStreamSynchronize(s) == hipSuccess;
    (void)hipHostFree(pin[0]);
    (void)hipHostFree(pin[1]);
    return ok;
}

} // namespace detail

#define T9_DIA_TRY(expr)                                                  \
    do {                                                                  \
        int _rc = (expr);                                                 \
        if (_rc != 0)                                                     \
            throw std::runtime_error(std::string(#expr) +                 \
                                     " failed rc=" + std::to_string(_rc)); \
    } while (0)

#define T9_DIA_HIP(expr)                                                  \
    do {                                                                  \
        hipError_t _e = (expr);                                           \
        if (_e != hipSuccess)                                             \
            throw std::runtime_error(std::string(#expr) + " failed: " +   \
                                     hipGetErrorString(_e));              \
    } while (0)

//! (key, value) pair for ReducePair — a POD TableItem (the reference's
//! pair<Key,Value> TableItem concept, core/reduce_table.hpp; std::pair is
//! not trivially copyable, so the GPU surface uses this layout-compatible
//! struct)
struct KeyValue {
    uint64_t key;
    uint64_t value;
    bool operator==(const KeyValue& o) const {
        return key == o.key && value == o.value;
    }
};
static_assert(sizeof(KeyValue) == 16, "KeyValue packing");

//! byte-lexicographic ascending order over a POD's bytes — the acceptance
//! comparator (TeraSort Record::operator< is its key-prefix restriction,
//! examples/terasort/terasort.cpp:35-37)
template <typename T>
struct LexicographicLess {
    bool operator()(const T& a, const T& b) const {
        return std::memcmp(&a, &b, sizeof(T)) < 0;
    }
};

//! Per-worker context (mirrors thrill api::Context services the hot path
//! consumes: my_rank/num_workers — api/context.hpp:243-245).
class Context {
public:
    explicit Context(int device = 0, int rank = 0, int world = 1,
                     void* rccl_comm = nullptr)
        : rank_(rank), world_(world) {
        T9_DIA_TRY(t9_create(&ctx_, device, rank, world, rccl_comm));
        T9_DIA_HIP(hipStreamCreate(&stream_));
    }
    ~Context() {
        if (stream_) (void)hipStreamDestroy(stream_);
        if (ctx_) t9_destroy(ctx_);
    }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;

    size_t my_rank() const { return rank_; }
    size_t num_workers() const { return world_; }
    t9_context* native() const { return ctx_; }
    hipStream_t stream() const { return stream_; }

    //! reference api/context.hpp consume mode (memory hint): accepted and
    //! ignored — DIAs here are explicit device buffers
    void enable_consume() {}

    //! scalar net services the examples touch (ctx.net.Barrier(),
    //! terasort.cpp:204): single-process no-ops; multi-rank scalar
    //! collectives run on the host control plane (pipeline.py) or a
    //! caller-provided communicator
    struct Net {
        void Barrier() {}
    } net;

private:
    t9_context* ctx_ = nullptr;
    hipStream_t stream_ = nullptr;
    int rank_, world_;
};

//! device buffer with shared ownership (DIAs are cheap handles, as the
//! reference's CountingPtr-refcounted nodes are)
struct DeviceBuf {
    void* ptr = nullptr;
    size_t bytes = 0;
    explicit DeviceBuf(size_t b) : bytes(b) {
        if (b) T9_DIA_HIP(hipMalloc(&ptr, b));
    }
    ~DeviceBuf() {
        if (ptr) (void)hipFree(ptr);
    }
};

//! Items that live on the GPU: fixed-size POD, raw-copied
//! (data/serialization.hpp:35-48 contract). Non-POD items (std::string
//! lines/words — the word_count tokenizer input) are held host-side, as
//! in the reference where string handling is CPU code fused into PreOp
//! chains; the DOp that consumes them
//! (ReduceByKey) dictionary-encodes and moves fixed-width work to the
//! GPU.
template <typename ValueType>
class DIA {
    static constexpr bool kDevice =
        std::is_trivially_copyable<ValueType>::value;

public:
    DIA() = default;
    DIA(Context* ctx, std::shared_ptr<DeviceBuf> buf, size_t n)
        : ctx_(ctx), buf_(buf), n_(n) {}
    DIA(Context* ctx, std::shared_ptr<std::vector<ValueType> > host)
        : ctx_(ctx), hvec_(host), n_(host ? host->size() : 0) {}

    size_t Size() const {
        // reference: ActionNode + AllReduce (api/size.hpp:64-69); world=1
        // here, so the local count is the global count
        return n_;
    }

    std::vector<ValueType> AllGather() const {
        if (hvec_) return *hvec_;
        std::vector<ValueType> out(n_);
        if (n_)
            T9_DIA_HIP(hipMemcpy(out.data(), buf_->ptr,
                                 n_ * sizeof(ValueType),
                                 hipMemcpyDeviceToHost));
        return out;
    }

    //! Sort with the default ascending order (reference api/sort.hpp:811:
    //! std::less; for byte-key PODs the acceptance order is
    //! LexicographicLess). Only these two comparator types are executable
    //! on the GPU path; anything else fails to compile, by design
    //! (INTEGRATION.md "Error behaviour").
    DIA Sort() const { return SortImpl(); }

    //! SortStable (reference api/sort.hpp:900-937): the radix pipeline is
    //! stable at every level, so Sort already implements the stable
    //! contract (sort_node_test.cpp:291-404's "lower source index wins").
    DIA SortStable() const { return SortImpl(); }

    template <typename Compare>
    DIA SortStable(const Compare& c) const { return Sort(c); }

    template <typename Compare>
    DIA Sort(const Compare&) const {
        static_assert(
            std::is_same<Compare, LexicographicLess<ValueType> >::value ||
                (std::is_same<Compare, std::less<ValueType> >::value &&
                 std::is_same<ValueType, uint64_t>::value),
            "GPU Sort supports LexicographicLess<T> (byte order) or "
            "std::less<uint64_t>");
        return SortImpl();
    }

    template <typename F>
    auto Map(const F& f) const
        -> DIA<typename std::result_of<F(ValueType)>::type> {
        // host-side map (the reference fuses Maps into PreOp chains on the
        // CPU — dia.hpp:358-405; tokenizers etc. stay CPU per SURVEY §3b)
        using Out = typename std::result_of<F(ValueType)>::type;
        auto in = AllGather();
        std::vector<Out> out;
        out.reserve(in.size());
        for (auto& v : in) out.push_back(f(v));
        return FromVector(*ctx_, out);
    }

    //! FlatMap — reference api/dia.hpp:405 (template on the output type,
    //! user lambda receives (item, emit)): host code, exactly as the
    //! reference fuses it into the CPU PreOp chain; the DOp that follows
    //! runs on the GPU.
    template <typename Out, typename F>
    DIA<Out> FlatMap(const F& f) const {
        auto in = AllGather();
        auto out = std::make_shared<std::vector<Out> >();
        auto emit = [&](const Out& o) { out->push_back(o); };
        for (auto& v : in) f(v, emit);
        return FromVector(*ctx_, *out);
    }

    //! ReduceByKey — reference api/reduce_by_key.hpp:241-463: reduce items
    //! with equal key_extractor(item) using the associative+commutative
    //! reduce_function; output order arbitrary (word_count_test.cpp:73-74).
    //! Implemented for pair<std::string, integral> items (the word_count
    //! shape): words are dictionary-encoded into two independent 64-bit
    //! hashes and reduced on the GPU 128-bit composite table
    //! (t9_reduce128_*; string identity per DESIGN.md — forced single-hash
    //! collisions stay separate). The u64-sum hot path is used when the
    //! user's reduce_function is additive on the counter — verified by
    //! ALGEBRAIC PROBING (the functor is a pure function of POD-ish pairs:
    //! it is evaluated on sample values and must return the counter sum,
    //! the shape word_count.hpp:50-53 has). min and max on the counter,
    //! with the key preserved, are recognised the same way and run on the
    //! device through t9_reduce128_*_op (a signed counter in signed
    //! order); a functor that is none of the three falls back to a host
    //! fold with the user's functor.
    template <typename KeyExtractor, typename ReduceFn>
    DIA<ValueType> ReduceByKey(const KeyExtractor& key_ex,
                               const ReduceFn& red) const;

    //! PrefixSum / ExPrefixSum — reference api/dia.hpp:1837-1868,
    //! api/prefix_sum.hpp:92-110: out[i] = initial ⊕ x[0] ⊕ … ⊕ x[i]
    //! (inclusive) or … ⊕ x[i-1] (exclusive, out[0] = initial). The
    //! functor is classified by ALGEBRAIC PROBING, as ReduceByKey's is.
    //! Items of type uint64_t / size_t, int64_t or double with a functor
    //! that is +, min or max (but not + over double) are scanned on the
    //! device by t9_scan_u64 and stay there; DIA<KeyValue>::PrefixSum with
    //! a functor of the shape { b.key, op(a.value, b.value) } — the
    //! prefix_doubling.cpp:346-351 idiom — runs t9_scan_kv. min and max
    //! over double follow the IEEE-754 totalOrder of the device
    //! (-0.0 < +0.0, NaNs at the ends). Everything else (a foreign
    //! functor, + over double, ExPrefixSum over KeyValue, other item
    //! types) folds sequentially on the host in the reference's own
    //! evaluation order.
    template <typename SumFunction = std::plus<ValueType> >
    DIA PrefixSum(const SumFunction& sum_function = SumFunction(),
                  const ValueType& initial_element = ValueType()) const {
        return ScanImpl(sum_function, initial_element, false);
    }
    template <typename SumFunction = std::plus<ValueType> >
    DIA ExPrefixSum(const SumFunction& sum_function = SumFunction(),
                    const ValueType& initial_element = ValueType()) const {
        return ScanImpl(sum_function, initial_element, true);
    }

    //! AllReduce / Sum / Min / Max actions — reference api/dia.hpp:599-752,
    //! api/all_reduce.hpp: without an initial value the fold starts from
    //! the first item and an empty DIA yields ValueType()
    //! (all_reduce.hpp:39-46); with one, it is folded in once, in front.
    //! Device execution (t9_fold_u64) under the conditions of PrefixSum's
    //! scalar case, host fold otherwise.
    template <typename ReduceFunction>
    ValueType AllReduce(const ReduceFunction& reduce_function) const {
        return FoldImpl(reduce_function, nullptr);
    }
    template <typename ReduceFunction>
    ValueType AllReduce(const ReduceFunction& reduce_function,
                        const ValueType& initial_value) const {
        return FoldImpl(reduce_function, &initial_value);
    }
    template <typename SumFunction = std::plus<ValueType> >
    ValueType Sum(const SumFunction& sum_function = SumFunction()) const {
        return FoldImpl(sum_function, nullptr);
    }
    template <typename SumFunction = std::plus<ValueType> >
    ValueType Sum(const SumFunction& sum_function,
                  const ValueType& initial_value) const {
        return FoldImpl(sum_function, &initial_value);
    }
    ValueType Min() const { return FoldImpl(MinFn(), nullptr); }
    ValueType Min(const ValueType& initial_value) const {
        return FoldImpl(MinFn(), &initial_value);
    }
    ValueType Max() const { return FoldImpl(MaxFn(), nullptr); }
    ValueType Max(const ValueType& initial_value) const {
        return FoldImpl(MaxFn(), &initial_value);
    }

    //! WriteBinary — reference api/write_binary.hpp: the items as packed
    //! binary (the POD raw-copy wire format, data/serialization.hpp:35-48),
    //! one file per worker: pathbase + zero-padded rank. The on-disk bytes
    //! are bit-compatible with the reference's files (terasort.cpp:184-200
    //! file mode).
    void WriteBinary(const std::string& pathbase) const {
        static_assert(std::is_trivially_copyable<ValueType>::value,
                      "WriteBinary needs fixed-size POD items");
        char name[512];
        std::snprintf(name, sizeof(name), "%s%010zu", pathbase.c_str(),
                      ctx_->my_rank());
        if (buf_ && n_) {
            // device-resident items: O_DIRECT + pinned ping-pong
            // (HBM -> disk without the pageable-copy throttle)
            if (detail::write_device_direct(name, buf_->ptr,
                                            n_ * sizeof(ValueType),
                                            ctx_->stream()))
                return;
        }
        auto host = AllGather();
        const size_t bytes = host.size() * sizeof(ValueType);
        if (detail::write_file_direct(name, host.data(), bytes))
            return;
        // buffered fallback (O_DIRECT unsupported on this filesystem)
        std::FILE* f = std::fopen(name, "wb");
        if (!f) throw std::runtime_error("WriteBinary: cannot open " +
                                         std::string(name));
        if (!host.empty() &&
            std::fwrite(host.data(), sizeof(ValueType), host.size(), f) !=
                host.size()) {
            std::fclose(f);
            throw std::runtime_error("WriteBinary: short write");
        }
        std::fclose(f);
    }

    Context& context() const { return *ctx_; }
    void* device_ptr() const { return buf_ ? buf_->ptr : nullptr; }

private:
    DIA SortImpl() const;

    //! common::minimum / maximum of the reference (std::min / std::max)
    struct MinFn {
        ValueType operator()(const ValueType& a, const ValueType& b) const {
            return std::min(a, b);
        }
    };
    struct MaxFn {
        ValueType operator()(const ValueType& a, const ValueType& b) const {
            return std::max(a, b);
        }
    };
    template <typename Fn>
    DIA ScanImpl(const Fn& fn, const ValueType& initial, bool exclusive) const;
    template <typename Fn>
    ValueType FoldImpl(const Fn& fn, const ValueType* initial) const;

    template <typename T>
    friend DIA<T> FromVector(Context&, const std::vector<T>&);

    Context* ctx_ = nullptr;
    std::shared_ptr<DeviceBuf> buf_;
    std::shared_ptr<std::vector<ValueType> > hvec_;  // non-POD host items
    size_t n_ = 0;
};

template <typename T>
typename std::enable_if<std::is_trivially_copyable<T>::value,
                        DIA<T> >::type
FromVectorImpl(Context& ctx, const std::vector<T>& v) {
    auto buf = std::make_shared<DeviceBuf>(v.size() * sizeof(T));
    if (!v.empty())
        T9_DIA_HIP(hipMemcpy(buf->ptr, v.data(), v.size() * sizeof(T),
                             hipMemcpyHostToDevice));
    return DIA<T>(&ctx, buf, v.size());
}

template <typename T>
typename std::enable_if<!std::is_trivially_copyable<T>::value,
                        DIA<T> >::type
FromVectorImpl(Context& ctx, const std::vector<T>& v) {
    return DIA<T>(&ctx, std::make_shared<std::vector<T> >(v));
}

template <typename T>
DIA<T> FromVector(Context& ctx, const std::vector<T>& v) {
    return FromVectorImpl<T>(ctx, v);
}

//! Generate — reference api/generate.hpp:37: DIA of generator(i) for
//! i in [0, size). The generator runs on the host (it is user code);
//! the DOps that follow run on the GPU.
template <typename Generator>
auto Generate(Context& ctx, size_t size, Generator gen)
    -> DIA<decltype(gen(size_t(0)))> {
    // generator taken by value and callable non-const, as the
    // reference's GeneratorFunction is (api/generate.hpp:37; stateful
    // rngs like terasort's GenerateRecord mutate)
    using T = decltype(gen(size_t(0)));
    std::vector<T> v;
    v.reserve(size);
    for (size_t i = 0; i < size; ++i) v.push_back(gen(i));
    return FromVector(ctx, v);
}

template <typename ValueType>
DIA<ValueType> DIA<ValueType>::SortImpl() const {
    static_assert(std::is_trivially_copyable<ValueType>::value,
                  "GPU Sort needs fixed-size POD items "
                  "(data/serialization.hpp:35-48 raw-copy contract)");
    constexpr size_t R = sizeof(ValueType);
    static_assert(R % 4 == 0, "record size must be a multiple of 4");
    auto out = std::make_shared<DeviceBuf>(n_ * R);
    if (n_) {
        if (std::is_same<ValueType, uint64_t>::value) {
            // keys are numeric u64: in-place radix of a copy
            T9_DIA_HIP(hipMemcpyAsync(out->ptr, buf_->ptr, n_ * 8,
                                      hipMemcpyDeviceToDevice,
                                      ctx_->stream()));
            DeviceBuf ws(t9_sort_u64_workspace(n_));
            T9_DIA_TRY(t9_sort_u64(ctx_->native(), (uint64_t*)out->ptr, n_,
                                   ws.ptr, ctx_->stream()));
            T9_DIA_HIP(hipStreamSynchronize(ctx_->stream()));
        }
        else {
            DeviceBuf ws(t9_sort_records_workspace(n_, R));
            T9_DIA_TRY(t9_sort_records(ctx_->native(),
                                       (const uint8_t*)buf_->ptr,
                                       (uint8_t*)out->ptr, n_, R,
                                       /*key_len*/ R, ws.ptr,
                                       ctx_->stream()));
            T9_DIA_HIP(hipStreamSynchronize(ctx_->stream()));
        }
    }
    return DIA(ctx_, out, n_);
}

//! ReducePair for (u64 key, u64 value) pairs with u64-sum reduction — the
//! reference's ReducePair (api/reduce_by_key.hpp:393-463) restricted to
//! the GPU-executable contract; word_count's (hash(word), count) pairs are
//! exactly this shape. Output order is arbitrary, as the
//! reference documents for reducing (word_count_test.cpp:73-74).
inline DIA<KeyValue> ReducePair(const DIA<KeyValue>& input,
                                uint64_t salt = 0) {
    using KV = KeyValue;
    Context& ctx = input.context();
    size_t n = input.Size();
    // SoA split ON DEVICE: the pairs are interleaved u64s, i.e. 16-byte
    // records with a u64 field at offset 0 (the key) and offset 8 (the
    // value) — two t9_extract_key64_le passes split them without any
    // host round trip (round-1 split staged through host vectors).
    DeviceBuf dk(n * 8), dv(n * 8), didx(n * 4);
    if (n) {
        T9_DIA_TRY(t9_extract_key64_le(ctx.native(),
                                       (const uint8_t*)input.device_ptr(),
                                       n, 16, 0, (uint64_t*)dk.ptr,
                                       (uint32_t*)didx.ptr, ctx.stream()));
        T9_DIA_TRY(t9_extract_key64_le(ctx.native(),
                                       (const uint8_t*)input.device_ptr(),
                                       n, 16, 8, (uint64_t*)dv.ptr,
                                       (uint32_t*)didx.ptr, ctx.stream()));
    }
    uint64_t cap = 1024;
    while (cap < 2 * n + 2) cap <<= 1;   // no grow/spill: size for 2x
    DeviceBuf tbl(2 * (cap + 1) * 8);   // interleaved (key, sum) slots
    DeviceBuf ok((cap + 1) * 8), ov((cap + 1) * 8);
    DeviceBuf derr(4), dn(8);
    hipStream_t s = ctx.stream();
    T9_DIA_TRY(t9_reduce_init(ctx.native(), (uint64_t*)tbl.ptr, cap, s));
    T9_DIA_TRY(t9_reduce_build(ctx.native(), (const uint64_t*)dk.ptr,
                               (const uint64_t*)dv.ptr, n,
                               (uint64_t*)tbl.ptr, cap,
                               salt, (uint32_t*)derr.ptr, s));
    T9_DIA_TRY(t9_reduce_drain(ctx.native(), (const uint64_t*)tbl.ptr,
                               cap,
                               (uint64_t*)ok.ptr, (uint64_t*)ov.ptr,
                               (uint64_t*)dn.ptr, s));
    uint64_t m = 0, err = 0;
    uint32_t err32 = 0;
    T9_DIA_HIP(hipMemcpy(&m, dn.ptr, 8, hipMemcpyDeviceToHost));
    T9_DIA_HIP(hipMemcpy(&err32, derr.ptr, 4, hipMemcpyDeviceToHost));
    err = err32;
    if (err) throw std::runtime_error("ReducePair: table overflow");
    std::vector<uint64_t> rk(m), rv(m);
    if (m) {
        T9_DIA_HIP(hipMemcpy(rk.data(), ok.ptr, m * 8,
                             hipMemcpyDeviceToHost));
        T9_DIA_HIP(hipMemcpy(rv.data(), ov.ptr, m * 8,
                             hipMemcpyDeviceToHost));
    }
    std::vector<KV> out(m);
    for (size_t i = 0; i < m; ++i) out[i] = KV{ rk[i], rv[i] };
    return FromVector(ctx, out);
}

//! The reduce functions that run on the device (t9_reduce_*_op): the
//! reference takes any associative (V, V) -> V
//! (core/reduce_probing_hash_table.hpp:233); these three have a native
//! 64-bit atomic.
enum class ReduceOp { Sum, Min, Max };

namespace detail {

//! Classify a reduce function by ALGEBRAIC PROBING: `apply(a, b)` — the
//! user's functor seen as (u64 bits, u64 bits) -> u64 bits — is evaluated
//! on operand pairs that tell sum, min and max apart (swapped operands, an
//! equal pair, a wide value, and a pair whose order differs between signed
//! and unsigned reading) and must agree with one operator on all of them.
//! Returns false for a functor that is none of the three.
template <typename Apply>
bool classify_reduce(const Apply& apply, bool is_signed, ReduceOp* op) {
    static const uint64_t probes[][2] = {
        { 3, 17 }, { 17, 3 }, { 5, 5 }, { 1ull << 40, 7 }, { 0, 9 },
        { ~0ull - 4, 2 },   // signed: -5 vs 2
    };
    bool sum = true, mn = true, mx = true;
    for (const auto& p : probes) {
        const uint64_t a = p[0], b = p[1], r = apply(a, b);
        const bool a_less = is_signed ? (int64_t)a < (int64_t)b : a < b;
        sum = sum && r == a + b;
        mn = mn && r == (a_less ? a : b);
        mx = mx && r == (a_less ? b : a);
    }
    if (sum) *op = ReduceOp::Sum;
    else if (mn) *op = ReduceOp::Min;
    else if (mx) *op = ReduceOp::Max;
    return sum || mn || mx;
}

inline int native_op(ReduceOp op) {
    return op == ReduceOp::Sum ? T9_OP_SUM
         : op == ReduceOp::Min ? T9_OP_MIN : T9_OP_MAX;
}

} // namespace detail

//! ReducePair with a reduce function — the reference's signature
//! (api/reduce_by_key.hpp:393-463). The functor is probed on
//! (u64, u64) -> u64 and must be +, min or max; the reduce then runs on
//! the device (t9_reduce_*_op). Anything else throws
//! std::invalid_argument: there is no host fold here.
template <typename ReduceFn,
          typename = decltype(std::declval<const ReduceFn&>()(
              uint64_t(), uint64_t()))>
DIA<KeyValue> ReducePair(const DIA<KeyValue>& input, const ReduceFn& red,
                         uint64_t salt = 0) {
    using KV = KeyValue;
    ReduceOp rop;
    if (!detail::classify_reduce(
            [&](uint64_t a, uint64_t b) { return (uint64_t)red(a, b); },
            false, &rop))
        throw std::invalid_argument(
            "ReducePair: the reduce function is none of +, min, max");
    const int op = detail::native_op(rop);
    Context& ctx = input.context();
    size_t n = input.Size();
    DeviceBuf dk(n * 8), dv(n * 8), didx(n * 4);
    if (n) {
        T9_DIA_TRY(t9_extract_key64_le(ctx.native(),
                                       (const uint8_t*)input.device_ptr(),
                                       n, 16, 0, (uint64_t*)dk.ptr,
                                       (uint32_t*)didx.ptr, ctx.stream()));
        T9_DIA_TRY(t9_extract_key64_le(ctx.native(),
                                       (const uint8_t*)input.device_ptr(),
                                       n, 16, 8, (uint64_t*)dv.ptr,
                                       (uint32_t*)didx.ptr, ctx.stream()));
    }
    uint64_t cap = 1024;
    while (cap < 2 * n + 2) cap <<= 1;   // no grow/spill: size for 2x
    DeviceBuf tbl(2 * (cap + 1) * 8);
    DeviceBuf ok((cap + 1) * 8), ov((cap + 1) * 8);
    DeviceBuf derr(4), dn(8);
    hipStream_t s = ctx.stream();
    T9_DIA_TRY(t9_reduce_init_op(ctx.native(), (uint64_t*)tbl.ptr, cap, op,
                                 T9_VAL_U64, s));
    T9_DIA_TRY(t9_reduce_build_op(ctx.native(), (const uint64_t*)dk.ptr,
                                  (const uint64_t*)dv.ptr, n,
                                  (uint64_t*)tbl.ptr, cap, salt, op,
                                  T9_VAL_U64, (uint32_t*)derr.ptr, s));
    T9_DIA_TRY(t9_reduce_drain_op(ctx.native(), (const uint64_t*)tbl.ptr,
                                  cap, op, T9_VAL_U64, (uint64_t*)ok.ptr,
                                  (uint64_t*)ov.ptr, (uint64_t*)dn.ptr, s));
    uint64_t m = 0;
    uint32_t err = 0;
    T9_DIA_HIP(hipMemcpy(&m, dn.ptr, 8, hipMemcpyDeviceToHost));
    T9_DIA_HIP(hipMemcpy(&err, derr.ptr, 4, hipMemcpyDeviceToHost));
    if (err) throw std::runtime_error("ReducePair: table overflow");
    std::vector<uint64_t> rk(m), rv(m);
    if (m) {
        T9_DIA_HIP(hipMemcpy(rk.data(), ok.ptr, m * 8,
                             hipMemcpyDeviceToHost));
        T9_DIA_HIP(hipMemcpy(rv.data(), ov.ptr, m * 8,
                             hipMemcpyDeviceToHost));
    }
    std::vector<KV> out(m);
    for (size_t i = 0; i < m; ++i) out[i] = KV{ rk[i], rv[i] };
    return FromVector(ctx, out);
}

//! ReduceToIndex — reference api/dia.hpp:1346-1351: keys are indices in
//! [0, size); entry i of the result is the reduced value of key i, or
//! `neutral` if no item has that key (the neutral element is not folded
//! in — core/reduce_by_index_post_phase.hpp:150-172). Runs over
//! t9_reduce_by_index_op with a probed +, min or max functor; anything
//! else throws std::invalid_argument, a key >= size std::out_of_range.
//! Deviation from the reference: it returns the whole reduced ITEMS (and a
//! neutral item) in index order; this surface returns the u64 VALUES, the
//! key being the position.
template <typename ReduceFn>
DIA<uint64_t> ReduceToIndex(const DIA<KeyValue>& input, const ReduceFn& red,
                            size_t size, uint64_t neutral = 0) {
    ReduceOp rop;
    if (!detail::classify_reduce(
            [&](uint64_t a, uint64_t b) { return (uint64_t)red(a, b); },
            false, &rop))
        throw std::invalid_argument(
            "ReduceToIndex: the reduce function is none of +, min, max");
    const int op = detail::native_op(rop);
    Context& ctx = input.context();
    const size_t n = input.Size();
    auto dense = std::make_shared<DeviceBuf>(size * 8);
    if (size == 0) return DIA<uint64_t>(&ctx, dense, 0);
    DeviceBuf dk(n * 8), dv(n * 8), didx(n * 4);
    if (n) {
        T9_DIA_TRY(t9_extract_key64_le(ctx.native(),
                                       (const uint8_t*)input.device_ptr(),
                                       n, 16, 0, (uint64_t*)dk.ptr,
                                       (uint32_t*)didx.ptr, ctx.stream()));
        T9_DIA_TRY(t9_extract_key64_le(ctx.native(),
                                       (const uint8_t*)input.device_ptr(),
                                       n, 16, 8, (uint64_t*)dv.ptr,
                                       (uint32_t*)didx.ptr, ctx.stream()));
    }
    DeviceBuf ws(t9_reduce_by_index_op_workspace(size)), derr(4);
    T9_DIA_TRY(t9_reduce_by_index_op(
        ctx.native(), (const uint64_t*)dk.ptr, (const uint64_t*)dv.ptr, n,
        0, size, op, T9_VAL_U64, neutral, (uint64_t*)dense->ptr,
        (uint32_t*)derr.ptr, ws.ptr, ctx.stream()));
    uint32_t err = 0;
    T9_DIA_HIP(hipMemcpy(&err, derr.ptr, 4, hipMemcpyDeviceToHost));
    if (err) throw std::out_of_range("ReduceToIndex: key >= size");
    return DIA<uint64_t>(&ctx, dense, size);
}

namespace detail {

//! 64-bit scalars the scan family runs on the device, and their
//! t9_val_type
template <typename T>
struct scan_scalar {
    static constexpr bool value =
        (std::is_integral<T>::value && sizeof(T) == 8 &&
         !std::is_same<T, bool>::value) ||
        std::is_same<T, double>::value;
    static constexpr int vtype =
        std::is_same<T, double>::value ? T9_VAL_F64
        : std::is_signed<T>::value     ? T9_VAL_I64
                                       : T9_VAL_U64;
};

template <typename T>
inline uint64_t scan_bits(const T& v) {
    static_assert(sizeof(T) == 8, "64-bit scalar");
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}
template <typename T>
inline T scan_value(uint64_t b) {
    static_assert(sizeof(T) == 8, "64-bit scalar");
    T v;
    std::memcpy(&v, &b, 8);
    return v;
}

//! classify_reduce for a functor over a 64-bit scalar. Integers are
//! probed on their bit patterns in their own signedness; doubles are
//! probed ON DOUBLES, including {-2, -1}, whose order is the opposite of
//! the integer order of the bits, signed or unsigned.
template <typename T, typename Fn>
bool classify_scalar(const Fn& fn, ReduceOp* op) {
    if constexpr (std::is_same<T, double>::value) {
        static const double probes[][2] = {
            { 3.0, 17.0 }, { 17.0, 3.0 }, { 5.0, 5.0 }, { -2.0, -1.0 },
            { 1e300, 7.0 }, { 0.5, -0.25 },
        };
        bool sum = true, mn = true, mx = true;
        for (const auto& p : probes) {
            const double a = p[0], b = p[1], r = (double)fn(a, b);
            sum = sum && r == a + b;
            mn = mn && r == (a < b ? a : b);
            mx = mx && r == (a < b ? b : a);
        }
        if (sum) *op = ReduceOp::Sum;
        else if (mn) *op = ReduceOp::Min;
        else if (mx) *op = ReduceOp::Max;
        return sum || mn || mx;
    }
    else {
        return classify_reduce(
            [&](uint64_t a, uint64_t b) {
                return (uint64_t)(T)fn((T)a, (T)b);
            },
            std::is_signed<T>::value, op);
    }
}

//! is fn(a, b) == { b.key, op(a.value, b.value) } with op one of +, min,
//! max? Probed on pairs with distinct keys.
template <typename Fn>
bool classify_kv_scan(const Fn& fn, ReduceOp* op) {
    bool key_kept = true;
    const bool known = classify_reduce(
        [&](uint64_t a, uint64_t b) {
            const KeyValue r = fn(KeyValue{ 0x1111, a },
                                  KeyValue{ 0x2222 + a, b });
            key_kept = key_kept && r.key == 0x2222 + a;
            return r.value;
        },
        false, op);
    return known && key_kept;
}

} // namespace detail

template <typename ValueType>
template <typename Fn>
DIA<ValueType> DIA<ValueType>::ScanImpl(const Fn& fn,
                                        const ValueType& initial,
                                        bool exclusive) const {
    if constexpr (detail::scan_scalar<ValueType>::value) {
        ReduceOp rop;
        constexpr int vt = detail::scan_scalar<ValueType>::vtype;
        if (!hvec_ && detail::classify_scalar<ValueType>(fn, &rop) &&
            !(rop == ReduceOp::Sum && vt == T9_VAL_F64)) {
            auto out = std::make_shared<DeviceBuf>(n_ * 8);
            if (n_) {
                DeviceBuf ws(t9_scan_workspace(n_));
                T9_DIA_TRY(t9_scan_u64(
                    ctx_->native(), (const uint64_t*)buf_->ptr,
                    (uint64_t*)out->ptr, n_, detail::native_op(rop), vt,
                    exclusive ? 1 : 0, detail::scan_bits(initial), nullptr,
                    ws.ptr, ctx_->stream()));
                T9_DIA_HIP(hipStreamSynchronize(ctx_->stream()));
            }
            return DIA(ctx_, out, n_);
        }
    }
    if constexpr (std::is_same<ValueType, KeyValue>::value) {
        ReduceOp rop;
        if (!exclusive && !hvec_ && detail::classify_kv_scan(fn, &rop)) {
            auto out = std::make_shared<DeviceBuf>(n_ * 16);
            if (n_) {
                DeviceBuf ws(t9_scan_workspace(n_));
                T9_DIA_TRY(t9_scan_kv(
                    ctx_->native(), (const uint8_t*)buf_->ptr,
                    (uint8_t*)out->ptr, n_, detail::native_op(rop),
                    T9_VAL_U64, initial.value, nullptr, ws.ptr,
                    ctx_->stream()));
                T9_DIA_HIP(hipStreamSynchronize(ctx_->stream()));
            }
            return DIA(ctx_, out, n_);
        }
    }
    // host fold with the user's functor, in the reference's order
    // (api/prefix_sum.hpp:92-110)
    const auto items = AllGather();
    std::vector<ValueType> out;
    out.reserve(items.size());
    ValueType sum = initial;
    for (const auto& x : items) {
        if (exclusive) out.push_back(sum);
        sum = fn(sum, x);
        if (!exclusive) out.push_back(sum);
    }
    return FromVector(*ctx_, out);
}

template <typename ValueType>
template <typename Fn>
ValueType DIA<ValueType>::FoldImpl(const Fn& fn,
                                   const ValueType* initial) const {
    if (n_ == 0) return initial ? *initial : ValueType();
    if constexpr (detail::scan_scalar<ValueType>::value) {
        ReduceOp rop;
        constexpr int vt = detail::scan_scalar<ValueType>::vtype;
        if (!hvec_ && detail::classify_scalar<ValueType>(fn, &rop) &&
            !(rop == ReduceOp::Sum && vt == T9_VAL_F64)) {
            DeviceBuf ws(t9_scan_workspace(n_)), dres(8);
            T9_DIA_TRY(t9_fold_u64(ctx_->native(),
                                   (const uint64_t*)buf_->ptr, n_, 1,
                                   detail::native_op(rop), vt,
                                   (uint64_t*)dres.ptr, ws.ptr,
                                   ctx_->stream()));
            uint64_t bits = 0;
            T9_DIA_HIP(hipMemcpyAsync(&bits, dres.ptr, 8,
                                      hipMemcpyDeviceToHost,
                                      ctx_->stream()));
            T9_DIA_HIP(hipStreamSynchronize(ctx_->stream()));
            const ValueType r = detail::scan_value<ValueType>(bits);
            return initial ? (ValueType)fn(*initial, r) : r;
        }
    }
    // host fold (api/all_reduce.hpp:56-64): from the initial value if
    // there is one, else from the first item
    const auto items = AllGather();
    size_t i = 0;
    ValueType sum = initial ? *initial : items[i++];
    for (; i < items.size(); ++i) sum = fn(sum, items[i]);
    return sum;
}

namespace detail {

//! the framework's string hash pair: fnv-1a under two bases, mixed by
//! Hash128to64 with two salts (DESIGN.md "config-4 string identity"; the
//! reference's std::hash is implementation-defined and affects placement
//! only). Sentinels remapped as t9_hash2_of does.
inline uint64_t fnv1a64(const char* s, size_t n, uint64_t basis) {
    uint64_t h = basis;
    for (size_t i = 0; i < n; ++i)
        h = (h ^ (uint8_t)s[i]) * 0x100000001B3ull;
    return h;
}

inline uint64_t mix128to64(uint64_t upper, uint64_t lower) {
    const uint64_t k = 0x9DDFEA08EB382D69ull;
    uint64_t a = (lower ^ upper) * k;
    a ^= (a >> 47);
    uint64_t b = (upper ^ a) * k;
    b ^= (b >> 47);
    b *= k;
    return b;
}

inline void string_hash2(const std::string& w, uint64_t* h1,
                         uint64_t* h2) {
    uint64_t a = mix128to64(0x9AE16A3B2F90404Full,
                            fnv1a64(w.data(), w.size(),
                                    0xCBF29CE484222325ull));
    uint64_t b = mix128to64(0xC3A5C85C97CB3127ull,
                            fnv1a64(w.data(), w.size(),
                                    0x84222325CBF29CE4ull));
    if (a == ~0ull) a ^= 1;
    if (b == ~0ull) b ^= 1;
    *h1 = a;
    *h2 = b;
}

} // namespace detail

//! ReduceByKey for (std::string word, integral count) pairs — the
//! word_count shape (examples/word_count/word_count.hpp:35-56). See the
//! declaration for the contract; the GPU path is
//! dictionary-encode -> t9_reduce128 (sum) -> decode.
template <typename ValueType>
template <typename KeyExtractor, typename ReduceFn>
DIA<ValueType> DIA<ValueType>::ReduceByKey(const KeyExtractor& key_ex,
                                           const ReduceFn& red) const {
    using Pair = ValueType;   // pair<std::string, Count>
    using Count = decltype(Pair().second);
    static_assert(std::is_integral<Count>::value && sizeof(Count) == 8,
                  "GPU ReduceByKey carries a 64-bit counter value");
    auto items = AllGather();
    const size_t n = items.size();

    // algebraic probe: is the user's reduce function "add the counters"?
    // (it is a pure function of its operands; probe a few samples)
    bool additive = true;
    for (uint64_t a : { 3ull, 17ull, 1ull << 40 }) {
        Pair x{ "probe", (Count)a }, y{ "probe", (Count)(a * 2 + 5) };
        Pair r = red(x, y);
        if ((uint64_t)r.second != a + (a * 2 + 5) || r.first != "probe") {
            additive = false;
            break;
        }
    }

    // not additive: is it min or max on .second with .first preserved?
    // Those run on the device too (t9_reduce128_*_op); a signed Count
    // reduces in two's-complement order.
    ReduceOp rop = ReduceOp::Sum;
    bool first_kept = true;
    const bool minmax =
        !additive &&
        detail::classify_reduce(
            [&](uint64_t a, uint64_t b) {
                Pair r = red(Pair{ "probe", (Count)a },
                             Pair{ "probe", (Count)b });
                first_kept = first_kept && r.first == "probe";
                return (uint64_t)r.second;
            },
            std::is_signed<Count>::value, &rop) &&
        first_kept && rop != ReduceOp::Sum;

    // dictionary-encode: word -> (h1, h2); keep the decode map. The
    // decode key folds (h1, h2) into one u64 — a fold collision
    // (p ~= 2^-64 per pair) would mis-map a word at DECODE time only;
    // the reduce itself separates on the full 128-bit composite
    // (DESIGN.md "Config-4 string identity").
    std::vector<uint64_t> k1(n), k2(n), vals(n);
    std::unordered_map<uint64_t, std::string> decode;
    for (size_t i = 0; i < n; ++i) {
        const std::string key = key_ex(items[i]);
        detail::string_hash2(key, &k1[i], &k2[i]);
        vals[i] = (uint64_t)items[i].second;
        decode.emplace(k1[i] ^ (k2[i] << 1 | k2[i] >> 63), key);
    }

    std::vector<Pair> out;
    if (n && additive) {
        // GPU 128-bit composite sum-reduce
        DeviceBuf d1(n * 8), d2(n * 8), dv(n * 8);
        T9_DIA_HIP(hipMemcpy(d1.ptr, k1.data(), n * 8,
                             hipMemcpyHostToDevice));
        T9_DIA_HIP(hipMemcpy(d2.ptr, k2.data(), n * 8,
                             hipMemcpyHostToDevice));
        T9_DIA_HIP(hipMemcpy(dv.ptr, vals.data(), n * 8,
                             hipMemcpyHostToDevice));
        uint64_t cap = 1024;
        while (cap < 2 * n + 2) cap <<= 1;
        DeviceBuf tbl(t9_reduce128_table_words(cap) * 8);
        DeviceBuf o1(cap * 8), o2(cap * 8), ov(cap * 8);
        DeviceBuf derr(4), dn(8);
        hipStream_t s = ctx_->stream();
        T9_DIA_TRY(t9_reduce128_init(ctx_->native(), (uint64_t*)tbl.ptr,
                                     cap, s));
        T9_DIA_TRY(t9_reduce128_build(ctx_->native(),
                                      (const uint64_t*)d1.ptr,
                                      (const uint64_t*)d2.ptr,
                                      (const uint64_t*)dv.ptr, n,
                                      (uint64_t*)tbl.ptr, cap, 0,
                                      (uint32_t*)derr.ptr, s));
        T9_DIA_TRY(t9_reduce128_drain(ctx_->native(),
                                      (const uint64_t*)tbl.ptr, cap,
                                      (uint64_t*)o1.ptr, (uint64_t*)o2.ptr,
                                      (uint64_t*)ov.ptr, (uint64_t*)dn.ptr,
                                      s));
        uint64_t m = 0;
        uint32_t err = 0;
        T9_DIA_HIP(hipMemcpy(&m, dn.ptr, 8, hipMemcpyDeviceToHost));
        T9_DIA_HIP(hipMemcpy(&err, derr.ptr, 4, hipMemcpyDeviceToHost));
        if (err) throw std::runtime_error("ReduceByKey: table overflow");
        std::vector<uint64_t> r1(m), r2(m), rv(m);
        if (m) {
            T9_DIA_HIP(hipMemcpy(r1.data(), o1.ptr, m * 8,
                                 hipMemcpyDeviceToHost));
            T9_DIA_HIP(hipMemcpy(r2.data(), o2.ptr, m * 8,
                                 hipMemcpyDeviceToHost));
            T9_DIA_HIP(hipMemcpy(rv.data(), ov.ptr, m * 8,
                                 hipMemcpyDeviceToHost));
        }
        out.reserve(m);
        for (uint64_t i = 0; i < m; ++i)
            out.push_back(Pair{
                decode.at(r1[i] ^ (r2[i] << 1 | r2[i] >> 63)),
                (Count)rv[i] });
    }
    else if (n && minmax) {
        // GPU 128-bit composite min/max-reduce
        const int op = detail::native_op(rop);
        const int vt = std::is_signed<Count>::value ? T9_VAL_I64
                                                    : T9_VAL_U64;
        DeviceBuf d1(n * 8), d2(n * 8), dv(n * 8);
        T9_DIA_HIP(hipMemcpy(d1.ptr, k1.data(), n * 8,
                             hipMemcpyHostToDevice));
        T9_DIA_HIP(hipMemcpy(d2.ptr, k2.data(), n * 8,
                             hipMemcpyHostToDevice));
        T9_DIA_HIP(hipMemcpy(dv.ptr, vals.data(), n * 8,
                             hipMemcpyHostToDevice));
        uint64_t cap = 1024;
        while (cap < 2 * n + 2) cap <<= 1;
        DeviceBuf tbl(t9_reduce128_table_words(cap) * 8);
        DeviceBuf o1(cap * 8), o2(cap * 8), ov(cap * 8);
        DeviceBuf derr(4), dn(8);
        hipStream_t s = ctx_->stream();
        T9_DIA_TRY(t9_reduce128_init_op(ctx_->native(), (uint64_t*)tbl.ptr,
                                        cap, op, vt, s));
        T9_DIA_TRY(t9_reduce128_build_op(
            ctx_->native(), (const uint64_t*)d1.ptr,
            (const uint64_t*)d2.ptr, (const uint64_t*)dv.ptr, n,
            (uint64_t*)tbl.ptr, cap, 0, op, vt, (uint32_t*)derr.ptr, s));
        T9_DIA_TRY(t9_reduce128_drain_op(
            ctx_->native(), (const uint64_t*)tbl.ptr, cap, op, vt,
            (uint64_t*)o1.ptr, (uint64_t*)o2.ptr, (uint64_t*)ov.ptr,
            (uint64_t*)dn.ptr, s));
        uint64_t m = 0;
        uint32_t err = 0;
        T9_DIA_HIP(hipMemcpy(&m, dn.ptr, 8, hipMemcpyDeviceToHost));
        T9_DIA_HIP(hipMemcpy(&err, derr.ptr, 4, hipMemcpyDeviceToHost));
        if (err) throw std::runtime_error("ReduceByKey: table overflow");
        std::vector<uint64_t> r1(m), r2(m), rv(m);
        if (m) {
            T9_DIA_HIP(hipMemcpy(r1.data(), o1.ptr, m * 8,
                                 hipMemcpyDeviceToHost));
            T9_DIA_HIP(hipMemcpy(r2.data(), o2.ptr, m * 8,
                                 hipMemcpyDeviceToHost));
            T9_DIA_HIP(hipMemcpy(rv.data(), ov.ptr, m * 8,
                                 hipMemcpyDeviceToHost));
        }
        out.reserve(m);
        for (uint64_t i = 0; i < m; ++i)
            out.push_back(Pair{
                decode.at(r1[i] ^ (r2[i] << 1 | r2[i] >> 63)),
                (Count)rv[i] });
    }
    else if (n) {
        // a reduce function that is none of +, min, max: host fold with
        // the user's functor (grouping semantics preserved)
        std::unordered_map<uint64_t, Pair> acc;
        for (size_t i = 0; i < n; ++i) {
            const uint64_t h = k1[i] ^ (k2[i] << 1 | k2[i] >> 63);
            auto it = acc.find(h);
            if (it == acc.end()) acc.emplace(h, items[i]);
            else it->second = red(it->second, items[i]);
        }
        out.reserve(acc.size());
        for (auto& kv : acc) out.push_back(kv.second);
    }
    return FromVector(*ctx_, out);
}

//! TextWordCount — word_count over raw text bytes with the whole PreOp on
//! the device: ReadLines + the WordCount split (a word is a maximal run of
//! bytes other than ' ' and '\n'), the string_hash2 pair, the 128-bit
//! composite reduce, and one spelling per group (the word's first
//! occurrence, sliced out of `text`). No decode map: identity is the
//! table's 128 bits end to end. Single rank, text.size() < 4 GiB. Returns a
//! host DIA, as ReduceByKey does; output order is arbitrary.
inline DIA<std::pair<std::string, size_t> >
TextWordCount(Context& ctx, const std::string& text) {
    using Pair = std::pair<std::string, size_t>;
    std::vector<Pair> out;
    const uint64_t nbytes = text.size();
    if (nbytes >= (1ull << 32))
        throw std::runtime_error("TextWordCount: input of 4 GiB or more");
    if (nbytes == 0) return FromVector(ctx, out);
    hipStream_t s = ctx.stream();
    t9_context* nat = ctx.native();

    DeviceBuf dtext(nbytes);
    T9_DIA_HIP(hipMemcpyAsync(dtext.ptr, text.data(), nbytes,
                              hipMemcpyHostToDevice, s));
    const uint64_t tok_cap = (nbytes + 1) / 2;
    DeviceBuf doff(tok_cap * 4), dlen(tok_cap * 4), dn(8), derr(4);
    DeviceBuf ws(t9_text_tokenize_workspace(nbytes));
    T9_DIA_TRY(t9_text_tokenize(nat, (const uint8_t*)dtext.ptr, nbytes,
                                (uint32_t*)doff.ptr, (uint32_t*)dlen.ptr,
                                (uint64_t*)dn.ptr, ws.ptr, s));
    uint64_t ntok = 0;
    T9_DIA_HIP(hipMemcpyAsync(&ntok, dn.ptr, 8, hipMemcpyDeviceToHost, s));
    T9_DIA_HIP(hipStreamSynchronize(s));
    if (ntok == 0) return FromVector(ctx, out);

    DeviceBuf d1(ntok * 8), d2(ntok * 8);
    T9_DIA_TRY(t9_text_hash2(nat, (const uint8_t*)dtext.ptr, nbytes,
                             (const uint32_t*)doff.ptr,
                             (const uint32_t*)dlen.ptr, ntok,
                             (uint64_t*)d1.ptr, (uint64_t*)d2.ptr,
                             (uint32_t*)derr.ptr, s));
    uint32_t herr = 0;
    T9_DIA_HIP(hipMemcpyAsync(&herr, derr.ptr, 4, hipMemcpyDeviceToHost, s));

    uint64_t cap = 1024;
    while (cap < 2 * ntok + 2) cap <<= 1;
    DeviceBuf tbl(t9_reduce128_table_words(cap) * 8);
    DeviceBuf o1(cap * 8), o2(cap * 8), ov(cap * 8);
    T9_DIA_TRY(t9_reduce128_init(nat, (uint64_t*)tbl.ptr, cap, s));
    T9_DIA_TRY(t9_reduce128_build(nat, (const uint64_t*)d1.ptr,
                                  (const uint64_t*)d2.ptr, nullptr, ntok,
                                  (uint64_t*)tbl.ptr, cap, 0,
                                  (uint32_t*)derr.ptr, s));
    T9_DIA_TRY(t9_reduce128_drain(nat, (const uint64_t*)tbl.ptr, cap,
                                  (uint64_t*)o1.ptr, (uint64_t*)o2.ptr,
                                  (uint64_t*)ov.ptr, (uint64_t*)dn.ptr, s));
    uint64_t m = 0;
    uint32_t err = 0;
    T9_DIA_HIP(hipMemcpyAsync(&m, dn.ptr, 8, hipMemcpyDeviceToHost, s));
    T9_DIA_HIP(hipMemcpyAsync(&err, derr.ptr, 4, hipMemcpyDeviceToHost, s));
    T9_DIA_HIP(hipStreamSynchronize(s));
    if (herr) throw std::runtime_error("TextWordCount: bad token range");
    if (err) throw std::runtime_error("TextWordCount: table overflow");
    if (m == 0) return FromVector(ctx, out);

    // slot of every token -> first token per slot -> the drained groups'
    // slots pick their representative; 4-byte records gathered by the
    // u32 slot / token number
    DeviceBuf dslot(ntok * 4), dfirst(cap * 4), dgslot(m * 4);
    DeviceBuf drep(m * 4), droff(m * 4), drlen(m * 4);
    T9_DIA_TRY(t9_reduce128_lookup(nat, (const uint64_t*)d1.ptr,
                                   (const uint64_t*)d2.ptr, ntok,
                                   (const uint64_t*)tbl.ptr, cap, 0,
                                   (uint32_t*)dslot.ptr, s));
    T9_DIA_TRY(t9_text_first_token(nat, (const uint32_t*)dslot.ptr, ntok,
                                   (uint32_t*)dfirst.ptr, cap, s));
    T9_DIA_TRY(t9_reduce128_lookup(nat, (const uint64_t*)o1.ptr,
                                   (const uint64_t*)o2.ptr, m,
                                   (const uint64_t*)tbl.ptr, cap, 0,
                                   (uint32_t*)dgslot.ptr, s));
    // every drained key is in the table, so its slot is a valid index
    // (checked on the host below before the dependent gathers' results
    // are used; an absent slot would index past dfirst)
    std::vector<uint32_t> gslot(m);
    T9_DIA_HIP(hipMemcpyAsync(gslot.data(), dgslot.ptr, m * 4,
                              hipMemcpyDeviceToHost, s));
    T9_DIA_HIP(hipStreamSynchronize(s));
    for (uint64_t i = 0; i < m; ++i)
        if (gslot[i] >= cap)
            throw std::runtime_error("TextWordCount: drained key not found");
    T9_DIA_TRY(t9_gather_records(nat, (const uint8_t*)dfirst.ptr,
                                 (const uint32_t*)dgslot.ptr, m, 4,
                                 (uint8_t*)drep.ptr, s));
    std::vector<uint32_t> rep(m);
    T9_DIA_HIP(hipMemcpyAsync(rep.data(), drep.ptr, m * 4,
                              hipMemcpyDeviceToHost, s));
    T9_DIA_HIP(hipStreamSynchronize(s));
    for (uint64_t i = 0; i < m; ++i)
        if (rep[i] >= ntok)
            throw std::runtime_error("TextWordCount: group without a token");
    T9_DIA_TRY(t9_gather_records(nat, (const uint8_t*)doff.ptr,
                                 (const uint32_t*)drep.ptr, m, 4,
                                 (uint8_t*)droff.ptr, s));
    T9_DIA_TRY(t9_gather_records(nat, (const uint8_t*)dlen.ptr,
                                 (const uint32_t*)drep.ptr, m, 4,
                                 (uint8_t*)drlen.ptr, s));
    std::vector<uint32_t> roff(m), rlen(m);
    std::vector<uint64_t> rv(m);
    T9_DIA_HIP(hipMemcpyAsync(roff.data(), droff.ptr, m * 4,
                              hipMemcpyDeviceToHost, s));
    T9_DIA_HIP(hipMemcpyAsync(rlen.data(), drlen.ptr, m * 4,
                              hipMemcpyDeviceToHost, s));
    T9_DIA_HIP(hipMemcpyAsync(rv.data(), ov.ptr, m * 8,
                              hipMemcpyDeviceToHost, s));
    T9_DIA_HIP(hipStreamSynchronize(s));
    out.reserve(m);
    for (uint64_t i = 0; i < m; ++i)
        out.emplace_back(text.substr(roff[i], rlen[i]), (size_t)rv[i]);
    return FromVector(ctx, out);
}

//! ReadBinary — reference api/read_binary.hpp: read packed fixed-size
//! items from files (the worker's share; world=1 here reads all).
template <typename T>
DIA<T> ReadBinary(Context& ctx, const std::vector<std::string>& files) {
    // device fast path (POD T): size the files, read each straight into
    // the device buffer via O_DIRECT + pinned staging (the pageable H2D
    // of the host-vector path measured ~2 GB/s)
    if (std::is_trivially_copyable<T>::value && !files.empty()) {
        size_t total = 0;
        bool sized = true;
        std::vector<size_t> sizes;
        for (const auto& path : files) {
            std::FILE* f = std::fopen(path.c_str(), "rb");
            if (!f) throw std::runtime_error("ReadBinary: cannot open " +
                                             path);
            std::fseek(f, 0, SEEK_END);
            long b = std::ftell(f);
            std::fclose(f);
            if (b < 0 || b % (long)sizeof(T)) {
                sized = false;
                break;
            }
            sizes.push_back((size_t)b);
            total += (size_t)b;
        }
        if (sized && total) {
            auto buf = std::make_shared<DeviceBuf>(total);
            size_t off = 0;
            bool ok = true;
            for (size_t i = 0; ok && i < files.size(); ++i) {
                ok = detail::read_device_direct(
                    files[i].c_str(), (char*)buf->ptr + off, sizes[i],
                    ctx.stream());
                off += sizes[i];
            }
            if (ok) return DIA<T>(&ctx, buf, total / sizeof(T));
            // else fall through to the host path
        }
    }
    std::vector<T> items;
    for (const auto& path : files) {
        std::FILE* f = std::fopen(path.c_str(), "rb");
        if (!f) throw std::runtime_error("ReadBinary: cannot open " + path);
        std::fseek(f, 0, SEEK_END);
        long bytes = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        if (bytes % (long)sizeof(T))
            throw std::runtime_error("ReadBinary: size not a multiple of "
                                     "the item size: " + path);
        size_t n = (size_t)bytes / sizeof(T);
        size_t old = items.size();
        items.resize(old + n);
        if (n) {
            std::fclose(f);
            f = nullptr;
            if (!detail::read_file_direct(path.c_str(),
                                          items.data() + old,
                                          n * sizeof(T))) {
                // buffered fallback
                f = std::fopen(path.c_str(), "rb");
                if (!f || std::fread(items.data() + old, sizeof(T), n,
                                     f) != n) {
                    if (f) std::fclose(f);
                    throw std::runtime_error("ReadBinary: short read");
                }
            }
        }
        if (f) std::fclose(f);
    }
    return FromVector(ctx, items);
}

//! GroupByKey — reference api/group_by_key.hpp (sort-based): sort the
//! pairs by key on the GPU, build the device group index
//! (t9_group_index), then apply the user's group function on the host per
//! group (user lambdas are host code in this surface). fn(key, vals_begin,
//! vals_end) -> Result.
template <typename Result, typename GroupFn>
std::vector<Result> GroupByKey(const DIA<KeyValue>& input,
                               const GroupFn& fn) {
    Context& ctx = input.context();
    auto host = input.AllGather();
    const size_t n = host.size();
    std::vector<uint64_t> hk(n), hv(n);
    for (size_t i = 0; i < n; ++i) {
        hk[i] = host[i].key;
        hv[i] = host[i].value;
    }
    std::vector<Result> out;
    if (n == 0) return out;
    DeviceBuf dk(n * 8), dv(n * 8), didx(n * 4), dsv(n * 8);
    DeviceBuf du(n * 8), doff(n * 8), dcnt(8);
    T9_DIA_HIP(hipMemcpy(dk.ptr, hk.data(), n * 8, hipMemcpyHostToDevice));
    T9_DIA_HIP(hipMemcpy(dv.ptr, hv.data(), n * 8, hipMemcpyHostToDevice));
    hipStream_t s = ctx.stream();
    {
        /* iota payload, sort (key, idx), gather values by idx */
        std::vector<uint32_t> iota(n);
        for (size_t i = 0; i < n; ++i) iota[i] = (uint32_t)i;
        T9_DIA_HIP(hipMemcpy(didx.ptr, iota.data(), n * 4,
                             hipMemcpyHostToDevice));
        DeviceBuf ws(t9_sort_pairs_workspace(n));
        T9_DIA_TRY(t9_sort_pairs_u64_u32(ctx.native(), (uint64_t*)dk.ptr,
                                         (uint32_t*)didx.ptr, n, ws.ptr,
                                         s));
        T9_DIA_TRY(t9_gather_records(ctx.native(), (const uint8_t*)dv.ptr,
                                     (const uint32_t*)didx.ptr, n, 8,
                                     (uint8_t*)dsv.ptr, s));
        DeviceBuf gws(t9_group_index_workspace(n));
        T9_DIA_TRY(t9_group_index(ctx.native(), (const uint64_t*)dk.ptr, n,
                                  (uint64_t*)du.ptr, (uint64_t*)doff.ptr,
                                  (uint64_t*)dcnt.ptr, gws.ptr, s));
        T9_DIA_HIP(hipStreamSynchronize(s));
    }
    uint64_t groups = 0;
    T9_DIA_HIP(hipMemcpy(&groups, dcnt.ptr, 8, hipMemcpyDeviceToHost));
    std::vector<uint64_t> uk(groups), off(groups), sv(n);
    T9_DIA_HIP(hipMemcpy(uk.data(), du.ptr, groups * 8,
                         hipMemcpyDeviceToHost));
    T9_DIA_HIP(hipMemcpy(off.data(), doff.ptr, groups * 8,
                         hipMemcpyDeviceToHost));
    T9_DIA_HIP(hipMemcpy(sv.data(), dsv.ptr, n * 8,
                         hipMemcpyDeviceToHost));
    out.reserve(groups);
    for (uint64_t g = 0; g < groups; ++g) {
        const uint64_t b = off[g];
        const uint64_t e = (g + 1 < groups) ? off[g + 1] : n;
        out.push_back(fn(uk[g], sv.data() + b, sv.data() + e));
    }
    return out;
}

//! InnerJoin — reference api/inner_join.hpp (sort-based, :213-287), in its
//! argument order: every pair of an item of `first` and an item of
//! `second` whose extracted keys are equal goes through join_fn. The key
//! extractors and join_fn are host code (as GroupByKey's group function
//! is); the matching runs on the device: t9_join_count / t9_join_emit on
//! the extracted keys give the index pairs (i, j), and the result is
//! join_fn(first[i], second[j]) in that order. A key is any integral type
//! of at most 64 bits and is compared by its 64-bit pattern (sign-extended
//! for signed types, so equal values have equal patterns).
//!
//! Deviation: the reference leaves the output order unspecified (its test
//! sorts before comparing); here it is deterministic — by key pattern
//! ascending as unsigned, then position in `first`, then position in
//! `second`. The reference's optional LocationDetection pre-pass is not
//! offered (it is off in the reference's default overload too).
template <typename First, typename Second, typename KeyExtractor1,
          typename KeyExtractor2, typename JoinFunction>
auto InnerJoin(const DIA<First>& first, const DIA<Second>& second,
               const KeyExtractor1& key_ex1, const KeyExtractor2& key_ex2,
               const JoinFunction& join_fn)
    -> DIA<typename std::decay<decltype(join_fn(
        std::declval<const First&>(),
        std::declval<const Second&>()))>::type> {
    using Key1 = typename std::decay<decltype(key_ex1(
        std::declval<const First&>()))>::type;
    using Key2 = typename std::decay<decltype(key_ex2(
        std::declval<const Second&>()))>::type;
    using Result = typename std::decay<decltype(join_fn(
        std::declval<const First&>(),
        std::declval<const Second&>()))>::type;
    static_assert(std::is_integral<Key1>::value && sizeof(Key1) <= 8 &&
                      std::is_integral<Key2>::value && sizeof(Key2) <= 8,
                  "GPU InnerJoin needs integral keys of at most 64 bits "
                  "(join wider keys on a hash and verify in join_fn)");
    Context& ctx = first.context();
    const auto a = first.AllGather();
    const auto b = second.AllGather();
    const size_t nl = a.size(), nr = b.size();
    std::vector<Result> out;
    if (nl == 0 || nr == 0) return FromVector(ctx, out);
    std::vector<uint64_t> lk(nl), rk(nr);
    for (size_t i = 0; i < nl; ++i) lk[i] = (uint64_t)key_ex1(a[i]);
    for (size_t j = 0; j < nr; ++j) rk[j] = (uint64_t)key_ex2(b[j]);
    DeviceBuf dl(nl * 8), dr(nr * 8), ws(t9_join_workspace(nl, nr));
    T9_DIA_HIP(hipMemcpy(dl.ptr, lk.data(), nl * 8, hipMemcpyHostToDevice));
    T9_DIA_HIP(hipMemcpy(dr.ptr, rk.data(), nr * 8, hipMemcpyHostToDevice));
    hipStream_t s = ctx.stream();
    uint64_t total = 0;
    T9_DIA_TRY(t9_join_count(ctx.native(), (const uint64_t*)dl.ptr, nl,
                             (const uint64_t*)dr.ptr, nr, &total, ws.ptr,
                             s));
    if (total == 0) return FromVector(ctx, out);
    DeviceBuf di(total * 4), dj(total * 4);
    T9_DIA_TRY(t9_join_emit(ctx.native(), nl, nr, ws.ptr, total,
                            (uint32_t*)di.ptr, (uint32_t*)dj.ptr, s));
    T9_DIA_HIP(hipStreamSynchronize(s));
    std::vector<uint32_t> li(total), ri(total);
    T9_DIA_HIP(hipMemcpy(li.data(), di.ptr, total * 4,
                         hipMemcpyDeviceToHost));
    T9_DIA_HIP(hipMemcpy(ri.data(), dj.ptr, total * 4,
                         hipMemcpyDeviceToHost));
    out.reserve(total);
    for (uint64_t p = 0; p < total; ++p)
        out.push_back(join_fn(a[li[p]], b[ri[p]]));
    return FromVector(ctx, out);
}

//! Merge — reference api/merge.hpp: merge sorted DIAs (u64, default
//! order); equal keys keep source order (a's before b's).
inline DIA<uint64_t> Merge(const DIA<uint64_t>& a, const DIA<uint64_t>& b) {
    Context& ctx = a.context();
    auto out = std::make_shared<DeviceBuf>((a.Size() + b.Size()) * 8);
    T9_DIA_TRY(t9_merge_u64(ctx.native(), (const uint64_t*)a.device_ptr(),
                            a.Size(), (const uint64_t*)b.device_ptr(),
                            b.Size(), (uint64_t*)out->ptr, ctx.stream()));
    T9_DIA_HIP(hipStreamSynchronize(ctx.stream()));
    return DIA<uint64_t>(&ctx, out, a.Size() + b.Size());
}

//! Merge for fixed-size POD records under the byte-lexicographic order
//! (the acceptance comparator; reference api/merge.hpp merges pre-sorted
//! DIAs with source order among equals — a's before b's)
template <typename T>
DIA<T> Merge(const DIA<T>& a, const DIA<T>& b) {
    static_assert(std::is_trivially_copyable<T>::value &&
                      sizeof(T) % 4 == 0,
                  "GPU Merge needs POD records, size % 4 == 0");
    Context& ctx = a.context();
    auto out = std::make_shared<DeviceBuf>((a.Size() + b.Size()) *
                                           sizeof(T));
    T9_DIA_TRY(t9_merge_records(
        ctx.native(), (const uint8_t*)a.device_ptr(), a.Size(),
        (const uint8_t*)b.device_ptr(), b.Size(), sizeof(T),
        (uint8_t*)out->ptr, ctx.stream()));
    T9_DIA_HIP(hipStreamSynchronize(ctx.stream()));
    return DIA<T>(&ctx, out, a.Size() + b.Size());
}

//! Run — reference api/context.cpp:947: construct the context(s) and run
//! the job. Round 1: one process, one GPU, rank 0.
inline int Run(const std::function<void(Context&)>& job) {
    Context ctx(0, 0, 1, nullptr);
    job(ctx);
    return 0;
}

} // namespace api

//! hoist the api entry points into t9::, as the reference hoists
//! thrill::api into thrill:: (each api header's `using api::X`), so
//! `using namespace t9` makes the example sources read identically
using api::Context;
using api::DIA;
using api::FromVector;
using api::Generate;
using api::GroupByKey;
using api::InnerJoin;
using api::KeyValue;
using api::Merge;
using api::ReadBinary;
using api::ReduceOp;
using api::ReducePair;
using api::ReduceToIndex;
using api::Run;

} // namespace t9
