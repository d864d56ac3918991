// TEST-ONLY program: the plan of the local predictor (csrc/ck_host.cpp: ck_host_local_needs, ck_host_local_plan) under
// -fsanitize=address,undefined (tests/test_local_plan_host.py builds and runs it; CPU only).
#include <stdio.h>

#include <random>

#include "ck_host.h"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
            return 1;                                                   \
        }                                                               \
    } while (0)

// the batches of one class: a partition in order, offsets = prefix sums, sums within max(budget, largest single need)
template <class Need, class Off>
static int verify_batches(const std::vector<std::pair<int64_t, int64_t>>& bt, int64_t n, long long cap, Need need, Off off,
                          long long* largest) {
    int64_t at = 0;
    for (const auto& b : bt) {
        CHECK(b.first == at && b.second > b.first);
        long long acc = 0;
        for (int64_t e = b.first; e < b.second; ++e) {
            CHECK(off(e) == acc && acc % 2 == 0);
            acc += need(e);
        }
        CHECK(acc <= cap);
        *largest = std::max(*largest, acc);
        at = b.second;
    }
    CHECK(at == n);
    return 0;
}

static int run(const std::vector<int>& cnt, int lds, int k_hi, int trend, long long budget) {
    const int64_t m = (int64_t)cnt.size();
    CkLocalNeeds nd;
    ck_host_local_needs(cnt.data(), m, lds, k_hi, trend, &nd);
    CkLocalPlan P;
    ck_host_local_plan(cnt.data(), nd, budget, trend, &P);
    CHECK((int64_t)nd.need.size() == m && (int64_t)P.off.size() == m && P.sys.size() == nd.tiled.size());
    int64_t n_tiled = 0;
    for (int64_t p = 0; p < m; ++p) {
        n_tiled += cnt[(size_t)p] > k_hi;
        CHECK((nd.need[(size_t)p] > 0) == (cnt[(size_t)p] > lds && cnt[(size_t)p] <= k_hi) && nd.need[(size_t)p] <= nd.need_max);
    }
    CHECK(n_tiled == (int64_t)nd.tiled.size());
    for (size_t t = 0; t < P.sys.size(); ++t) {
        const CkLocalSys& x = P.sys[t];
        CHECK(x.p == nd.tiled[t] && x.k == cnt[(size_t)x.p] && x.k > k_hi && x.kq % 64 == 0 && x.kq >= x.k + 2 + trend &&
              x.kq < x.k + 2 + trend + 64 && x.ld == x.kq + 128);
        CHECK(t == 0 || x.k < P.sys[t - 1].k || (x.k == P.sys[t - 1].k && x.p > P.sys[t - 1].p));
        CHECK(ck_local_tiled_doubles(x.k, trend) <= nd.need_max);
    }
    const long long cap = std::max(budget, nd.need_max);
    long long largest = 0;
    CHECK(verify_batches(P.batches, m, cap, [&](int64_t p) { return nd.need[(size_t)p]; }, [&](int64_t p) { return P.off[(size_t)p]; },
                         &largest) == 0);
    if (!P.sys.empty())
        CHECK(verify_batches(P.tbatches, (int64_t)P.sys.size(), cap, [&](int64_t t) { return ck_local_tiled_doubles(P.sys[(size_t)t].k, trend); },
                             [&](int64_t t) { return P.sys[(size_t)t].off; }, &largest) == 0);
    else
        CHECK(P.tbatches.empty());
    CHECK(P.slab_doubles == largest);
    return 0;
}

int main() {
    std::mt19937_64 rng(5);
    for (int trend : {0, 3})
        for (int k_hi : {60, 100, 140}) {   // below (the universal form), at and above the LDS limit of 100
            CHECK(run(std::vector<int>(9, 0), 100, k_hi, trend, 4096) == 0);
            CHECK(run({100, 101, k_hi, k_hi + 1, 0, 99}, 100, k_hi, trend, 4096) == 0);
            CHECK(run({137}, 100, k_hi, trend, 0) == 0);
            CHECK(run({120, 130, 110, 300, 300, 200}, 100, k_hi, trend, 1) == 0);   // below every single need
        }
    for (int it = 0; it < 300; ++it) {
        std::vector<int> cnt((size_t)(1 + rng() % (it == 0 ? 5000 : 300)));
        const int top = 1 + (int)(rng() % 500);
        for (auto& x : cnt) x = rng() % 4 == 0 ? 0 : (int)(rng() % (unsigned)top);
        CHECK(run(cnt, 100, 40 + (int)(rng() % 200), it % 2 ? 3 : 0, (long long)(rng() % 2000000)) == 0);
    }
    printf("all checks passed\n");
    return 0;
}
