/* scan_test.cpp — C++ surface tests of the scan family: PrefixSum /
 * ExPrefixSum and the Sum / Min / Max / AllReduce actions of t9::api::DIA.
 * The device path (t9_scan_u64 / t9_scan_kv / t9_fold_u64) is told from
 * the host fold by the "scan" perf class: it counts launches after a
 * device-eligible functor and none after a foreign one. Expectations are
 * sequential folds computed in-test. Needs a GPU.
 *
 * Build: hipcc scan_test.cpp -I../../include -L../../thrill_amd -lt9
 *   (done by __graft_entry__.build(); run by tests/test_gpu_scan_cxx.py
 *   from the repository root)
 */
#include <t9/dia.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
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

/* launches recorded under the "scan" perf class since the last call */
static uint64_t scan_launches() {
    double ms = 0;
    uint64_t n = 0;
    if (t9_perf_read("scan", &ms, &n) != 0) ++failures;
    t9_perf_reset();
    return n;
}

static uint64_t bits_of(double d) {
    uint64_t b;
    std::memcpy(&b, &d, 8);
    return b;
}

/* the reference's three known answers (operations_test.cpp:501-571) */
static void test_known_answers(api::Context& ctx) {
    auto integers = Generate(ctx, 16, [](size_t i) { return i; });
    scan_launches();

    std::vector<size_t> in = integers.PrefixSum(std::plus<size_t>(), 42)
                                 .AllGather();
    CHECK(scan_launches() > 0);
    CHECK(in.size() == 16);
    size_t ctr = 42;
    for (size_t i = 0; i < in.size(); ++i) {
        ctr += i;
        CHECK(in[i] == ctr);
    }

    std::vector<size_t> ex = integers.ExPrefixSum(std::plus<size_t>(), 42)
                                 .AllGather();
    CHECK(scan_launches() > 0);
    CHECK(ex.size() == 16);
    ctr = 42;
    for (size_t i = 0; i < ex.size(); ++i) {
        CHECK(ex[i] == ctr);
        ctr += i;
    }

    /* a multiply functor is none of +, min, max: host fold, and with the
     * default initial 0 every product is 0 */
    auto one_to_ten = Generate(ctx, 10, [](size_t i) { return i + 1; });
    std::vector<size_t> fac =
        one_to_ten.ExPrefixSum([](size_t a, size_t b) { return a * b; })
            .AllGather();
    CHECK(scan_launches() == 0);
    CHECK(fac.size() == 10);
    ctr = 0;
    for (size_t i = 0; i < fac.size(); ++i) {
        ctr *= i + 1;
        CHECK(fac[i] == ctr);
    }

    /* the default functor is + */
    std::vector<size_t> def = integers.PrefixSum().AllGather();
    CHECK(scan_launches() > 0);
    ctr = 0;
    for (size_t i = 0; i < def.size(); ++i) {
        ctr += i;
        CHECK(def[i] == ctr);
    }
}

/* signed min, double max on the device; double + on the host, bit for
 * bit the sequential sum */
static void test_signed_and_double(api::Context& ctx) {
    const size_t n = 10000;
    std::mt19937_64 rng(0x5CA9);
    std::vector<int64_t> si(n);
    std::vector<double> d(n);
    for (size_t i = 0; i < n; ++i) {
        si[i] = (int64_t)rng();
        d[i] = std::ldexp((double)(int64_t)rng(), (int)(rng() % 80) - 100);
    }
    scan_launches();

    auto smin = FromVector(ctx, si)
                    .PrefixSum([](int64_t a, int64_t b) {
                                   return std::min(a, b);
                               },
                               std::numeric_limits<int64_t>::max())
                    .AllGather();
    CHECK(scan_launches() > 0);
    int64_t m = std::numeric_limits<int64_t>::max();
    bool ok = smin.size() == n;
    for (size_t i = 0; ok && i < n; ++i) {
        m = std::min(m, si[i]);
        ok = smin[i] == m;
    }
    CHECK(ok);

    auto dmax = FromVector(ctx, d)
                    .ExPrefixSum([](double a, double b) {
                                     return std::max(a, b);
                                 },
                                 -1.5)
                    .AllGather();
    CHECK(scan_launches() > 0);
    double mx = -1.5;
    ok = dmax.size() == n;
    for (size_t i = 0; ok && i < n; ++i) {
        ok = bits_of(dmax[i]) == bits_of(mx);
        mx = std::max(mx, d[i]);
    }
    CHECK(ok);

    auto dsum = FromVector(ctx, d).PrefixSum(std::plus<double>(), 0.25)
                    .AllGather();
    CHECK(scan_launches() == 0);
    double acc = 0.25;
    ok = dsum.size() == n;
    for (size_t i = 0; ok && i < n; ++i) {
        acc = acc + d[i];
        ok = bits_of(dsum[i]) == bits_of(acc);
    }
    CHECK(ok);
}

/* the prefix-doubling idiom: names flow from each run start to its run */
static void test_keyvalue(api::Context& ctx) {
    const size_t n = 10000;
    std::mt19937_64 rng(0x1D0B);
    std::vector<api::KeyValue> kv(n);
    for (size_t i = 0; i < n; ++i)
        kv[i] = api::KeyValue{ rng(), (i == 0 || rng() % 7 == 0) ? i + 1
                                                                 : 0 };
    auto in = FromVector(ctx, kv);
    scan_launches();
    auto got = in.PrefixSum([](const api::KeyValue& a,
                               const api::KeyValue& b) {
                     return api::KeyValue{ b.key,
                                           std::max(a.value, b.value) };
                 }).AllGather();
    CHECK(scan_launches() > 0);
    bool ok = got.size() == n;
    uint64_t name = 0;
    for (size_t i = 0; ok && i < n; ++i) {
        name = std::max(name, kv[i].value);
        ok = got[i].key == kv[i].key && got[i].value == name;
    }
    CHECK(ok);

    /* a.key instead of b.key is not the device shape: host fold */
    auto keep_a = in.PrefixSum([](const api::KeyValue& a,
                                  const api::KeyValue& b) {
                        return api::KeyValue{ a.key, a.value + b.value };
                    }).AllGather();
    CHECK(scan_launches() == 0);
    uint64_t s = 0;
    ok = keep_a.size() == n;
    for (size_t i = 0; ok && i < n; ++i) {
        s += kv[i].value;
        ok = keep_a[i].key == 0 && keep_a[i].value == s;
    }
    CHECK(ok);

    /* exclusive over pairs stays on the host */
    auto ex = in.ExPrefixSum([](const api::KeyValue& a,
                                const api::KeyValue& b) {
                    return api::KeyValue{ b.key, a.value + b.value };
                }, api::KeyValue{ 7, 5 }).AllGather();
    CHECK(scan_launches() == 0);
    api::KeyValue run{ 7, 5 };
    ok = ex.size() == n;
    for (size_t i = 0; ok && i < n; ++i) {
        ok = ex[i] == run;
        run = api::KeyValue{ kv[i].key, run.value + kv[i].value };
    }
    CHECK(ok);
}

static void test_actions(api::Context& ctx) {
    const size_t n = 100000;
    std::mt19937_64 rng(0xAC71);
    std::vector<uint64_t> u(n);
    std::vector<int64_t> si(n);
    std::vector<double> d(n);
    uint64_t usum = 0;
    for (size_t i = 0; i < n; ++i) {
        u[i] = rng();
        usum += u[i];
        si[i] = (int64_t)rng();
        d[i] = (double)(int64_t)rng() / 1024.0;
    }
    auto du = FromVector(ctx, u);
    auto dsi = FromVector(ctx, si);
    auto dd = FromVector(ctx, d);
    scan_launches();

    CHECK(du.Sum() == usum);
    CHECK(scan_launches() > 0);
    CHECK(du.Sum(std::plus<uint64_t>(), 1000) == usum + 1000);
    CHECK(du.Min() == *std::min_element(u.begin(), u.end()));
    CHECK(du.Max() == *std::max_element(u.begin(), u.end()));
    CHECK(du.Min(0) == 0);
    CHECK(du.Max(~0ull) == ~0ull);
    CHECK(dsi.Min() == *std::min_element(si.begin(), si.end()));
    CHECK(dsi.Max() == *std::max_element(si.begin(), si.end()));
    CHECK(dsi.Max(std::numeric_limits<int64_t>::max()) ==
          std::numeric_limits<int64_t>::max());
    CHECK(dd.Min() == *std::min_element(d.begin(), d.end()));
    CHECK(dd.Max() == *std::max_element(d.begin(), d.end()));
    CHECK(du.AllReduce([](uint64_t a, uint64_t b) {
              return std::max(a, b);
          }) == *std::max_element(u.begin(), u.end()));
    CHECK(du.AllReduce(std::plus<uint64_t>(), 7) == usum + 7);
    CHECK(scan_launches() > 0);

    /* + over double and a foreign functor fold on the host */
    double dacc = d[0];
    for (size_t i = 1; i < n; ++i) dacc = dacc + d[i];
    CHECK(bits_of(dd.Sum()) == bits_of(dacc));
    uint64_t x = 5;
    for (size_t i = 0; i < n; ++i) x = x ^ u[i];
    CHECK(du.AllReduce([](uint64_t a, uint64_t b) { return a ^ b; }, 5) ==
          x);
    CHECK(scan_launches() == 0);

    /* an empty DIA: ValueType() without an initial value, the initial
     * value with one; the device is not asked */
    auto none = FromVector(ctx, std::vector<uint64_t>());
    CHECK(none.Sum() == 0);
    CHECK(none.Min() == 0);
    CHECK(none.Max() == 0);
    CHECK(none.Max(9) == 9);
    CHECK(none.Sum(std::plus<uint64_t>(), 11) == 11);
    CHECK(none.AllReduce(std::plus<uint64_t>()) == 0);
    CHECK(none.PrefixSum().Size() == 0);
    CHECK(none.ExPrefixSum(std::plus<uint64_t>(), 3).Size() == 0);
    CHECK(scan_launches() == 0);
}

int main() {
    t9_perf_enable(1);
    api::Context ctx;
    test_known_answers(ctx);
    test_signed_and_double(ctx);
    test_keyvalue(ctx);
    test_actions(ctx);
    t9_perf_enable(0);
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
