/* reduce_op_test.cpp — C++ surface tests of the reduce operators:
 * ReducePair with a reduce function, ReduceByKey with min/max on the
 * counter, ReduceToIndex with a neutral element. Every DOp runs on the GPU
 * through t9::api; expectations are std::map folds computed in-test.
 * Needs a GPU.
 *
 * Build: hipcc reduce_op_test.cpp -I../../include -L../../thrill_amd -lt9
 *   (done by __graft_entry__.build(); run by
 *   tests/test_gpu_reduce_ops_cxx.py from the repository root)
 */
#include <t9/dia.hpp>

#include <algorithm>
#include <cstdio>
#include <fstream>
#include <map>
#include <random>
#include <sstream>
#include <string>
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

/* the probe tells the three operators apart and rejects the rest */
static void test_probe() {
    ReduceOp op;
    auto u = [](auto f) {
        return [f](uint64_t a, uint64_t b) { return (uint64_t)f(a, b); };
    };
    CHECK(api::detail::classify_reduce(
              u([](uint64_t a, uint64_t b) { return a + b; }), false, &op) &&
          op == ReduceOp::Sum);
    CHECK(api::detail::classify_reduce(
              u([](uint64_t a, uint64_t b) { return std::min(a, b); }),
              false, &op) &&
          op == ReduceOp::Min);
    CHECK(api::detail::classify_reduce(
              u([](uint64_t a, uint64_t b) { return std::max(a, b); }),
              false, &op) &&
          op == ReduceOp::Max);
    CHECK(!api::detail::classify_reduce(
        u([](uint64_t a, uint64_t b) { return a * b; }), false, &op));
    CHECK(!api::detail::classify_reduce(
        u([](uint64_t a, uint64_t) { return a; }), false, &op));
    /* signed max read as unsigned is not a max */
    CHECK(!api::detail::classify_reduce(
        u([](uint64_t a, uint64_t b) {
            return (uint64_t)std::max((int64_t)a, (int64_t)b);
        }),
        false, &op));
}

/* ReducePair with min / max / + against a std::map fold: 100 000 pairs
 * over 601 keys (the reduce_pre_phase_test key count) */
static void test_reduce_pair_ops(api::Context& ctx) {
    const size_t n = 100000, mod = 601;
    std::mt19937_64 rng(0x0915);
    std::vector<api::KeyValue> pairs(n);
    std::map<uint64_t, uint64_t> emin, emax, esum;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t k = rng() % mod, v = rng();
        pairs[i] = api::KeyValue{ k, v };
        if (!emin.count(k)) {
            emin[k] = v;
            emax[k] = v;
        }
        emin[k] = std::min(emin[k], v);
        emax[k] = std::max(emax[k], v);
        esum[k] += v;
    }
    auto dia = api::FromVector(ctx, pairs);
    auto as_map = [](const api::DIA<api::KeyValue>& d) {
        std::map<uint64_t, uint64_t> m;
        auto out = d.AllGather();
        for (auto& kv : out) m[kv.key] = kv.value;
        CHECK(m.size() == out.size());
        return m;
    };
    CHECK(as_map(api::ReducePair(dia, [](uint64_t a, uint64_t b) {
              return std::min(a, b);
          })) == emin);
    CHECK(as_map(api::ReducePair(dia, [](uint64_t a, uint64_t b) {
              return std::max(a, b);
          })) == emax);
    CHECK(as_map(api::ReducePair(dia, [](uint64_t a, uint64_t b) {
              return a + b;
          })) == esum);
    /* the two-argument overload is still the sum */
    CHECK(as_map(api::ReducePair(dia)) == esum);
    CHECK(as_map(api::ReducePair(dia, 7)) == esum);

    bool threw = false;
    try {
        api::ReducePair(dia, [](uint64_t a, uint64_t b) { return a * b; });
    }
    catch (const std::invalid_argument&) {
        threw = true;
    }
    CHECK(threw);
}

/* ReduceByKey on (string, int64_t) with max / min on .second, negative
 * counts included: the device path in signed order */
static void test_reduce_by_key_signed(api::Context& ctx) {
    using P = std::pair<std::string, int64_t>;
    std::vector<P> items;
    std::map<std::string, int64_t> emax, emin;
    std::mt19937_64 rng(77);
    for (int i = 0; i < 20000; ++i) {
        std::string w = "w" + std::to_string(rng() % 97);
        int64_t v = (int64_t)(rng() % 2001) - 1000;
        if (i % 97 == 5) v = -1000000 - i;   /* some groups all-negative */
        items.push_back(P{ w, v });
        if (!emax.count(w)) {
            emax[w] = v;
            emin[w] = v;
        }
        emax[w] = std::max(emax[w], v);
        emin[w] = std::min(emin[w], v);
    }
    /* one group of negatives only */
    items.push_back(P{ "neg", -7 });
    items.push_back(P{ "neg", -3 });
    items.push_back(P{ "neg", -11 });
    emax["neg"] = -3;
    emin["neg"] = -11;
    auto dia = api::FromVector(ctx, items);
    auto keyx = [](const P& p) -> std::string { return p.first; };
    auto mx = dia.ReduceByKey(keyx, [](const P& a, const P& b) -> P {
        return P(a.first, std::max(a.second, b.second));
    });
    std::map<std::string, int64_t> got;
    for (auto& p : mx.AllGather()) got[p.first] = p.second;
    CHECK(got == emax);
    auto mn = dia.ReduceByKey(keyx, [](const P& a, const P& b) -> P {
        return P(a.first, std::min(a.second, b.second));
    });
    got.clear();
    for (auto& p : mn.AllGather()) got[p.first] = p.second;
    CHECK(got == emin);
}

/* the additive bacon-ipsum case still matches the reference's KAT table
 * (tests/golden/bacon_ipsum_correct.json: a flat {"word": count} object) */
static void test_bacon_ipsum_additive(api::Context& ctx) {
    using P = std::pair<std::string, size_t>;
    std::ifstream in("tests/golden/wordcount.in");
    CHECK(in.good());
    std::vector<P> items;
    std::string line;
    while (std::getline(in, line)) {
        std::stringstream ss(line);
        std::string w;
        while (std::getline(ss, w, ' '))
            if (!w.empty()) items.push_back(P{ w, 1 });
    }
    std::ifstream jf("tests/golden/bacon_ipsum_correct.json");
    CHECK(jf.good());
    std::stringstream js;
    js << jf.rdbuf();
    const std::string j = js.str();
    std::map<std::string, size_t> expect;
    size_t pos = 0;
    while ((pos = j.find('"', pos)) != std::string::npos) {
        const size_t end = j.find('"', pos + 1);
        const std::string word = j.substr(pos + 1, end - pos - 1);
        const size_t colon = j.find(':', end);
        expect[word] = (size_t)std::strtoull(j.c_str() + colon + 1,
                                             nullptr, 10);
        pos = colon;
    }
    CHECK(expect.size() == 71);
    auto red = api::FromVector(ctx, items)
                   .ReduceByKey(
                       [](const P& p) -> std::string { return p.first; },
                       [](const P& a, const P& b) -> P {
                           return P(a.first, a.second + b.second);
                       });
    std::map<std::string, size_t> got;
    for (auto& p : red.AllGather()) got[p.first] = p.second;
    CHECK(got == expect);
}

/* ReduceToIndex: min with a non-zero neutral; absent indices read the
 * neutral, an index holding only all-ones (min's identity) reads all-ones */
static void test_reduce_to_index(api::Context& ctx) {
    const size_t size = 1000, n = 50000;
    const uint64_t neutral = 12345;
    std::mt19937_64 rng(31);
    std::vector<api::KeyValue> pairs;
    std::vector<uint64_t> emin(size, neutral), esum(size, neutral);
    std::vector<bool> hit(size, false);
    for (size_t i = 0; i < n; ++i) {
        uint64_t k = rng() % size;
        if (k % 10 == 3 || k == 500) continue;   /* holes */
        const uint64_t v = rng() >> 8;
        pairs.push_back(api::KeyValue{ k, v });
        emin[k] = hit[k] ? std::min(emin[k], v) : v;
        esum[k] = hit[k] ? esum[k] + v : v;
        hit[k] = true;
    }
    pairs.push_back(api::KeyValue{ 500, ~0ull });
    emin[500] = ~0ull;
    esum[500] = ~0ull;
    auto dia = api::FromVector(ctx, pairs);
    auto mn = api::ReduceToIndex(
        dia, [](uint64_t a, uint64_t b) { return std::min(a, b); }, size,
        neutral);
    CHECK(mn.Size() == size);
    CHECK(mn.AllGather() == emin);
    auto sm = api::ReduceToIndex(
        dia, [](uint64_t a, uint64_t b) { return a + b; }, size, neutral);
    CHECK(sm.AllGather() == esum);

    bool threw = false;
    try {
        api::ReduceToIndex(
            dia, [](uint64_t a, uint64_t b) { return std::max(a, b); }, 400);
    }
    catch (const std::out_of_range&) {
        threw = true;
    }
    CHECK(threw);
}

int main() {
    return api::Run([](api::Context& ctx) {
        test_probe();
        test_reduce_pair_ops(ctx);
        test_reduce_by_key_signed(ctx);
        test_bacon_ipsum_additive(ctx);
        test_reduce_to_index(ctx);
        if (failures == 0)
            std::printf("reduce_op_test: all checks passed\n");
        else
            std::printf("reduce_op_test: %d FAILURES\n", failures);
        if (failures) std::exit(1);
    });
}
