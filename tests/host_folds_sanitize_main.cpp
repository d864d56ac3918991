// TEST-ONLY program: the fold layout of leave-group-out cross-validation (csrc/ck_host.cpp: ck_host_fold_plan) under
// -fsanitize=address,undefined (tests/test_cv_folds_host.py builds and runs it; CPU only).
#include <stdio.h>
#include <stdlib.h>

#include <numeric>
#include <random>

#include "ck_host.h"

extern "C" const char* ck_last_error(void);

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
            return 1;                                                   \
        }                                                               \
    } while (0)

static int verify(const CkFoldPlan& P, int n_folds) {
    CHECK((int)P.off.size() == n_folds + 1 && P.gpos.size() % 128 == 0);
    for (int f = 0; f < n_folds; ++f) {
        for (int q = P.off[f]; q < P.off[f + 1]; ++q) {
            CHECK(P.gpos[(size_t)(P.gbase[f] + q - P.off[f])] == P.pos[q]);
            CHECK(q == P.off[f] || P.pos[q] > P.pos[q - 1]);
            CHECK(P.pos[q] >= P.pmin && P.pos[q] <= P.pmax);
        }
    }
    long long end = 0;
    for (const CkFoldTile& t : P.tiles) {
        CHECK(t.a0 % 128 == 0 && t.b0 % 128 == 0 && t.a0 + 128 <= (int)P.gpos.size() && t.b0 <= t.a0);
        CHECK(t.c_off >= 0 && t.c_off + 127LL * t.ld + 128 <= P.buffer_doubles);
        for (int r = 0; r < 128; ++r) CHECK(P.gpos[(size_t)(t.a0 + r)] >= t.pos0);
        end = std::max(end, t.c_off);
    }
    for (const CkFoldBig& b : P.big) CHECK(b.off + (long long)(b.kq + 128) * b.ld + 8 * 64 * 64 <= P.buffer_doubles && b.kq >= 2 * b.s + 1);
    return 0;
}

int main() {
    std::mt19937_64 rng(7);
    const int64_t n[2] = {3000, 2500};
    const int64_t n0p = 3008;
    std::vector<int64_t> perm0(3000), perm1(2500);
    std::iota(perm0.begin(), perm0.end(), 0);
    std::iota(perm1.begin(), perm1.end(), 0);
    std::shuffle(perm0.begin(), perm0.end(), rng);
    std::shuffle(perm1.begin(), perm1.end(), rng);
    CkFoldPlan P;
    // random labels of 40 folds on both processes, some never withheld
    std::vector<int32_t> f0(3000), f1(2500);
    for (auto& x : f0) x = (int32_t)(rng() % 41) - 1;
    for (auto& x : f1) x = (int32_t)(rng() % 41) - 1;
    CHECK(ck_host_fold_plan(0, 2, n, n0p, perm0.data(), perm1.data(), f0.data(), f1.data(), 40, 4096, &P) == 0);
    CHECK(verify(P, 40) == 0);
    CHECK(ck_host_fold_plan(1, 2, n, n0p, perm0.data(), perm1.data(), f0.data(), f1.data(), 40, 4096, &P) == 0);
    CHECK(verify(P, 40) == 0);
    // singletons, the other process absent
    for (int a = 0; a < 3000; ++a) f0[a] = a;
    CHECK(ck_host_fold_plan(0, 2, n, n0p, perm0.data(), perm1.data(), f0.data(), nullptr, 3000, 4096, &P) == 0);
    CHECK(verify(P, 3000) == 0 && P.big.empty() && P.n_small_tiles == 24);
    // one fold of everything up to the cap, and one beyond it
    for (auto& x : f0) x = 0;
    CHECK(ck_host_fold_plan(0, 1, n, n0p, perm0.data(), nullptr, f0.data(), nullptr, 1, 3000, &P) == 0);
    CHECK(verify(P, 1) == 0 && P.big.size() == 1 && P.big[0].s == 3000);
    CHECK(ck_host_fold_plan(0, 1, n, n0p, perm0.data(), nullptr, f0.data(), nullptr, 1, 2999, &P) == -1);
    // refusals
    f0[5] = 1;
    CHECK(ck_host_fold_plan(0, 1, n, n0p, perm0.data(), nullptr, f0.data(), nullptr, 1, 4096, &P) == -1);
    CHECK(ck_host_fold_plan(0, 1, n, n0p, perm0.data(), nullptr, f0.data(), nullptr, 3, 4096, &P) == -1);
    CHECK(ck_host_fold_plan(0, 1, n, n0p, perm0.data(), nullptr, nullptr, nullptr, 3, 4096, &P) == -1);
    printf("last refusal: %s\n", ck_last_error());
    printf("all checks passed\n");
    return 0;
}
