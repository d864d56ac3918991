// TEST-ONLY program: the plan of cross-validation in the moving neighbourhood (csrc/ck_host.cpp: ck_host_local_cv_plan) under
// -fsanitize=address,undefined (tests/test_local_cv_folds_host.py builds and runs it; CPU only).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

// what the header promises of a plan, for process i with the labels fold_i (null: everything predicted)
static int verify(const CkLocalCvPlan& P, int i, const int64_t n[2], int64_t n0p, const int32_t* fold_i, const int32_t* fold_o,
                  int n_folds, const std::vector<int64_t>* perm) {
    const int64_t n_i = n[i];
    size_t m = 0;
    for (int64_t a = 0; a < n_i; ++a) {
        if (fold_i && fold_i[a] < 0) continue;
        CHECK(m < P.plist.size() && P.plist[m] == a && P.fp[m] == (fold_i ? fold_i[a] : -1));
        ++m;
    }
    CHECK(m == P.plist.size() && P.idx.size() == m && P.fp.size() == m);
    CHECK(P.n_groups == (fold_i ? n_folds : (n_i > 0 ? 1 : 0)) && (int64_t)P.off.size() == P.n_groups + 1);
    CHECK(P.off.front() == 0 && P.off.back() == (long long)m);
    std::vector<char> seen(m, 0);
    for (int64_t g = 0; g < P.n_groups; ++g)
        for (long long q = P.off[g]; q < P.off[g + 1]; ++q) {
            const int t = P.idx[q];
            CHECK(t >= 0 && (size_t)t < m && !seen[t]);
            seen[t] = 1;
            CHECK(q == P.off[g] || P.idx[q - 1] < t);
            if (fold_i) CHECK(P.fp[t] == g);
        }
    for (int f = 0; f < n_folds; ++f) {
        int64_t c = 0;
        for (int64_t a = 0; fold_i && a < n_i; ++a) c += fold_i[a] == f;
        for (int64_t a = 0; fold_o && a < n[1 - i]; ++a) c += fold_o[a] == f;
        CHECK(P.size[f] == c);
    }
    CHECK((int64_t)P.gself.size() == n[0] + n[1]);
    for (int k = 0; k < 2; ++k)
        for (int64_t j = 0; j < n[k]; ++j) CHECK(P.gself[(k ? n[0] : 0) + perm[k][j]] == (k ? n0p : 0) + j);
    return 0;
}

int main() {
    std::mt19937_64 rng(11);
    for (int64_t n0 : {1, 63, 64, 65, 257, 3000}) {
        const int64_t n[2] = {n0, n0 / 2 + 1};
        const int64_t n0p = (n0 + 63) / 64 * 64;
        std::vector<int64_t> perm[2];
        for (int k = 0; k < 2; ++k) {
            perm[k].resize((size_t)n[k]);
            std::iota(perm[k].begin(), perm[k].end(), 0);
            std::shuffle(perm[k].begin(), perm[k].end(), rng);
        }
        const int K = (int)std::min<int64_t>(7, n[1]);
        std::vector<int32_t> f[2];
        for (int k = 0; k < 2; ++k) {
            f[k].resize((size_t)n[k]);
            for (auto& x : f[k]) x = (int32_t)(rng() % (uint64_t)(K + 1)) - 1;
            for (int q = 0; q < K && q < n[k]; ++q) f[k][(size_t)q] = q;   // no fold without a datum of either process
        }
        const int Kb = (int)std::min<int64_t>(K, std::min(n[0], n[1]));
        if (Kb < K)
            for (int k = 0; k < 2; ++k)
                for (auto& x : f[k]) x = x >= Kb ? -1 : x;
        CkLocalCvPlan P;
        for (int i = 0; i < 2; ++i) {
            CHECK(ck_host_local_cv_plan("t", i, 2, n, n0p, perm[0].data(), perm[1].data(), f[0].data(), f[1].data(), Kb, false, &P) == 0);
            CHECK(verify(P, i, n, n0p, f[i].data(), f[1 - i].data(), Kb, perm) == 0);
            // the other process without labels; then no labels at all, under a buffer
            CHECK(ck_host_local_cv_plan("t", i, 2, n, n0p, perm[0].data(), perm[1].data(), i == 0 ? f[0].data() : nullptr,
                                        i == 1 ? f[1].data() : nullptr, Kb, false, &P) == 0);
            CHECK(verify(P, i, n, n0p, f[i].data(), nullptr, Kb, perm) == 0);
            CHECK(ck_host_local_cv_plan("t", i, 2, n, n0p, perm[0].data(), perm[1].data(), nullptr, nullptr, 0, true, &P) == 0);
            CHECK(verify(P, i, n, n0p, nullptr, nullptr, 0, perm) == 0);
            CHECK(ck_host_local_cv_plan("t", i, 2, n, n0p, perm[0].data(), perm[1].data(), nullptr, nullptr, 0, false, &P) == -1);
        }
        // singletons: one fold per datum of process 0
        std::vector<int32_t> s0((size_t)n0);
        std::iota(s0.begin(), s0.end(), 0);
        CHECK(ck_host_local_cv_plan("t", 0, 2, n, n0p, perm[0].data(), perm[1].data(), s0.data(), nullptr, (int32_t)n0, false, &P) == 0);
        CHECK(verify(P, 0, n, n0p, s0.data(), nullptr, (int)n0, perm) == 0);
        // refusals: a label out of range (named), a fold wholly in the other process, a negative fold count
        s0[(size_t)(n0 - 1)] = (int32_t)n0;
        CHECK(ck_host_local_cv_plan("t", 0, 2, n, n0p, perm[0].data(), perm[1].data(), s0.data(), nullptr, (int32_t)n0, false, &P) == -1);
        CHECK(strstr(ck_last_error(), ("datum " + std::to_string(n0 - 1) + " of process 0").c_str()) != nullptr);
        std::vector<int32_t> none((size_t)n0, -1), one((size_t)n[1], 0);
        CHECK(ck_host_local_cv_plan("t", 0, 2, n, n0p, perm[0].data(), perm[1].data(), none.data(), one.data(), 1, false, &P) == -1);
        CHECK(strstr(ck_last_error(), "fold 0 is empty") != nullptr);
        CHECK(ck_host_local_cv_plan("t", 0, 2, n, n0p, perm[0].data(), perm[1].data(), none.data(), nullptr, -1, false, &P) == -1);
    }
    printf("last refusal: %s\n", ck_last_error());
    printf("all checks passed\n");
    return 0;
}
