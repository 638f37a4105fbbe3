/* join_test.cpp — C++ surface test of t9::api::InnerJoin: the four shapes
 * of the reference's join test (unique keys, one key on both sides, one key
 * with sides of different sizes, two different item types), plus the
 * deterministic output order this surface adds, signed keys, an empty side
 * and sides without a common key. The "join_bounds" / "join_emit" perf
 * classes prove the matching ran on the device. Expectations are computed
 * in-test. Needs a GPU.
 *
 * Build: hipcc join_test.cpp -I../../include -L../../thrill_amd -lt9
 *   (done by __graft_entry__.build(); run by tests/test_gpu_join_cxx.py
 *   from the repository root)
 */
#include <t9/dia.hpp>

#include <cstdio>
#include <tuple>
#include <utility>
#include <vector>

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            ++failures;                                                   \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__,  \
                         #cond);                                          \
        }                                                                 \
    } while (0)

using namespace t9;

using Pair = std::pair<size_t, size_t>;
using Triple = std::tuple<size_t, size_t, size_t>;
using Quint = std::tuple<size_t, size_t, size_t, size_t, size_t>;

/* launches of one perf class since the last reset */
static uint64_t launches(const char* cls) {
    double ms = 0;
    uint64_t n = 0;
    if (t9_perf_read(cls, &ms, &n) != 0) ++failures;
    return n;
}

/* n unique keys on both sides: one row per key, already in key order */
static void test_unique_keys(Context& ctx) {
    const size_t n = 9999;
    /* descending on the left, so the output order is the join's doing */
    auto left = Generate(ctx, n, [n](size_t i) {
        const size_t k = n - 1 - i;
        return Pair(k, k * k);
    });
    auto right = Generate(ctx, n,
                          [](size_t i) { return Pair(i, i * i * i); });
    auto key = [](const Pair& p) { return p.first; };
    t9_perf_reset();
    auto joined = InnerJoin(
        left, right, key, key, [](const Pair& a, const Pair& b) {
            return Triple(a.first, a.second, b.second);
        });
    CHECK(launches("join_bounds") == 1);
    CHECK(launches("join_emit") == 1);
    std::vector<Triple> out = joined.AllGather();
    CHECK(out.size() == n);
    CHECK(joined.Size() == n);
    bool ok = out.size() == n;
    for (size_t i = 0; ok && i < n; ++i)
        ok = out[i] == Triple(i, i * i, i * i * i);
    CHECK(ok);
}

/* one key on both sides, m x n: the full product, left-major */
static void test_single_key(Context& ctx, size_t m, size_t n) {
    auto left = Generate(ctx, m, [](size_t i) { return Pair(1, i); });
    auto right = Generate(ctx, n, [](size_t i) { return Pair(1, i * i); });
    auto key = [](const Pair& p) { return p.first; };
    auto joined = InnerJoin(left, right, key, key,
                            [](const Pair& a, const Pair& b) {
                                return Pair(a.second, b.second);
                            });
    std::vector<Pair> out = joined.AllGather();
    CHECK(out.size() == m * n);
    bool ok = out.size() == m * n;
    for (size_t p = 0; ok && p < out.size(); ++p)
        ok = out[p] == Pair(p / n, (p % n) * (p % n));
    CHECK(ok);
}

/* items of two different types, two different extractors */
static void test_different_types(Context& ctx) {
    const size_t n = 9999;
    auto left = Generate(ctx, n, [](size_t i) { return Pair(i, i * i); });
    auto right = Generate(ctx, n, [](size_t i) {
        return Triple(i, i * i, i * i * i);
    });
    auto joined = InnerJoin(
        left, right, [](const Pair& p) { return p.first; },
        [](const Triple& t) { return std::get<0>(t); },
        [](const Pair& a, const Triple& b) {
            return Quint(a.first, a.second, std::get<0>(b), std::get<1>(b),
                         std::get<2>(b));
        });
    std::vector<Quint> out = joined.AllGather();
    CHECK(out.size() == n);
    bool ok = out.size() == n;
    for (size_t i = 0; ok && i < n; ++i)
        ok = out[i] == Quint(i, i * i, i, i * i, i * i * i);
    CHECK(ok);
}

/* POD items on the device, signed 32-bit keys, many-to-many: the order is
 * key pattern (negative keys sort last, as unsigned), then left position,
 * then right position */
struct Item {
    int32_t key;
    uint32_t tag;
};
static void test_order_and_signed_keys(Context& ctx) {
    std::vector<Item> l = { { 7, 0 }, { -1, 1 }, { 7, 2 }, { 0, 3 },
                            { -1, 4 }, { 5, 5 } };
    std::vector<Item> r = { { -1, 10 }, { 7, 11 }, { 9, 12 }, { 7, 13 },
                            { 0, 14 } };
    auto joined = InnerJoin(
        FromVector(ctx, l), FromVector(ctx, r),
        [](const Item& x) { return x.key; },
        [](const Item& x) { return x.key; },
        [](const Item& a, const Item& b) {
            return KeyValue{ a.tag, b.tag };
        });
    const std::vector<KeyValue> expect = {
        { 3, 14 },                                    /* key 0 */
        { 0, 11 }, { 0, 13 }, { 2, 11 }, { 2, 13 },   /* key 7 */
        { 1, 10 }, { 4, 10 },                         /* key -1 */
    };
    CHECK(joined.AllGather() == expect);
}

static void test_empty_and_disjoint(Context& ctx) {
    auto key = [](uint64_t x) { return x; };
    auto fn = [](uint64_t a, uint64_t b) { return a + b; };
    auto some = Generate(ctx, 100, [](size_t i) { return (uint64_t)(2 * i); });
    auto odd = Generate(ctx, 100,
                        [](size_t i) { return (uint64_t)(2 * i + 1); });
    auto none = FromVector(ctx, std::vector<uint64_t>());
    CHECK(InnerJoin(some, none, key, key, fn).Size() == 0);
    CHECK(InnerJoin(none, some, key, key, fn).Size() == 0);
    CHECK(InnerJoin(some, odd, key, key, fn).Size() == 0);
    /* every u64 value is a key: 0 and 2^64-1 join like any other */
    std::vector<uint64_t> e = { ~0ull, 0, 5, ~0ull };
    auto ends = FromVector(ctx, e);
    std::vector<uint64_t> got = InnerJoin(ends, ends, key, key, fn)
                                    .AllGather();
    const std::vector<uint64_t> expect = { 0, 10, ~0ull - 1, ~0ull - 1,
                                           ~0ull - 1, ~0ull - 1 };
    CHECK(got == expect);
}

int main() {
    try {
        Context ctx(0, 0, 1, nullptr);
        t9_perf_enable(1);
        test_unique_keys(ctx);
        t9_perf_reset();
        t9_perf_enable(0);
        test_single_key(ctx, 333, 333);
        test_single_key(ctx, 100, 333);
        test_single_key(ctx, 50, 333);
        test_different_types(ctx);
        test_order_and_signed_keys(ctx);
        test_empty_and_disjoint(ctx);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 2;
    }
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("join_test: all checks passed\n");
    return 0;
}
