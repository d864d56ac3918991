// TEST-ONLY program: the pure planning of the dense likelihood family (csrc/ck_host.cpp: ck_host_mem_admit,
// ck_host_fisher_plan, ck_host_reml_start) under -fsanitize=address,undefined (tests/test_lik_plan_host.py builds and runs it;
// CPU only).  Exactly sized buffers: a read or write past an end is the sanitizer's to report.
#include <math.h>
#include <stdio.h>

#include <random>
#include <vector>

#include "ck_host.h"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
            return 1;                                                   \
        }                                                               \
    } while (0)

int main() {
    // ---- the admission: amounts near the top of the 64-bit range's useful part (288 GB of memory, a 65 536-site Schur order)
    {
        const int64_t G = (int64_t)1 << 30;
        const CkMemState st = {288 * G, false, 0, 0, 10 * G, 4096, 2 * G};
        CkMemAdmit a = ck_host_mem_admit(st, {40 * G, 65536, 3 * G, 12345});
        CHECK(a.need == 40 * G + ck_host_schur_bytes(65536) + 3 * G + 12345);
        CHECK(a.avail == 288 * G + 10 * G + ck_host_schur_bytes(4096) + 2 * G && !a.arena_short);
        a = ck_host_mem_admit(st, {10 * G, 4096, 2 * G, 0});   // nothing grows
        CHECK(a.need == 0 && a.avail == 288 * G);
        const CkMemState ar = {G, true, 8 * G, 7 * G, 0, 0, 0};
        a = ck_host_mem_admit(ar, {2 * G, 0, 0, 0});
        CHECK(a.arena_short && a.need == 0 && a.avail == G);
        CHECK(ck_host_tri_bytes(512) == ck_host_panel_payload(512, 0) && ck_host_schur_bytes(0) == 0);
    }
    // ---- the Fisher plan: every subset of the operand classes, rooms from nothing to everything
    for (int n_procs = 1; n_procs <= 2; ++n_procs)
        for (int64_t n0p : {333, 384, 512, 700}) {
            const int64_t Np = n_procs == 1 ? 1024 : 1536;
            const int nK = (int)(Np / CK_HOST_NB);
            for (unsigned mask = 0; mask < (1u << CK_HOST_FISHER_NOPS); mask += 37) {
                bool live[CK_HOST_FISHER_NOPS];
                for (int a = 0; a < CK_HOST_FISHER_NOPS; ++a) live[a] = (mask >> a & 1u) && (n_procs == 2 || a < 4 || a == 11);
                CkFisherPlan full;
                CHECK(ck_host_fisher_plan(n_procs, Np, n0p, nK, live, INT64_MAX / 2, 3, 11, 0, &full) == 0);
                CHECK(full.groups.size() == 1 && full.region == full.b_total);
                for (int64_t room : {(int64_t)-1, (int64_t)0, full.fixed_bytes, full.fixed_bytes + 16 * full.b_max,
                                     full.fixed_bytes + 8 * full.b_total - 8, full.fixed_bytes + 8 * full.b_total}) {
                    CkFisherPlan P;
                    const int rc = ck_host_fisher_plan(n_procs, Np, n0p, nK, live, room, 3, 11, 0, &P);
                    CHECK(P.fixed_bytes == full.fixed_bytes && P.d_total == full.d_total && P.units.size() == full.units.size());
                    if (rc) {
                        CHECK(P.groups.empty() && P.region == 0);
                        continue;
                    }
                    int seen[CK_HOST_FISHER_NOPS] = {};
                    for (const auto& g : P.groups) {
                        int64_t s = 0;
                        for (int a : g) ++seen[a], s += P.b_doubles[a];
                        CHECK(s <= P.region);
                    }
                    for (int a = 0; a < CK_HOST_FISHER_NOPS; ++a) CHECK(seen[a] == (live[a] && a < CK_HOST_FOP_DIAG0 ? 1 : 0));
                    CHECK(P.region * 8 * (P.groups.size() > 1 ? 2 : 1) <= room - P.fixed_bytes || P.b_total == 0);
                }
            }
        }
    // ---- the REML start vectors on exactly sized arrays
    std::mt19937_64 rng(5);
    std::normal_distribution<double> nd;
    for (int p : {1, 2, 16}) {
        const int q = 1 + p;
        const int64_t Np = 96;
        std::vector<double> W((size_t)((q + Np) * (q + 1))), beta((size_t)p), R((size_t)p * p, 0.0), av((size_t)q * Np, NAN);
        for (auto& x : W) x = nd(rng);
        for (auto& x : beta) x = nd(rng);
        for (int j = 0; j < p; ++j) {
            for (int l = 0; l < j; ++l) R[(size_t)(j * p + l)] = 0.1 * nd(rng);
            R[(size_t)(j * p + j)] = 1.0 + 0.1 * j;
        }
        ck_host_reml_start(p, Np, W.data(), q, beta.data(), R.data(), av.data());
        for (int64_t r = 0; r < Np; ++r) {   // R C_r = B_r, row by row
            const double* wr = &W[(size_t)((q + r) * (q + 1))];
            double a = wr[1];
            for (int j = 0; j < p; ++j) a -= wr[2 + j] * beta[(size_t)j];
            CHECK(fabs(av[(size_t)r] - a) <= 1e-12 * (1.0 + fabs(a)));
            for (int j = 0; j < p; ++j) {
                double s = 0.0;
                for (int l = 0; l <= j; ++l) s += R[(size_t)(j * p + l)] * av[(size_t)(1 + l) * Np + r];
                CHECK(fabs(s - wr[2 + j]) <= 1e-10 * (1.0 + fabs(wr[2 + j])));
            }
        }
    }
    printf("all checks passed\n");
    return 0;
}
