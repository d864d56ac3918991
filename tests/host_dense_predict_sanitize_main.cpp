// TEST-ONLY program: the dense predictors' host arithmetic (csrc/ck_host.cpp: ck_host_block_members, ck_host_prior_pieces,
// ck_host_block_chunk, ck_host_draw_chunk, ck_host_coincident_site, ck_host_universal_finish, and ck_host_local_block_layout
// on top of the first) under -fsanitize=address,undefined (tests/test_dense_predict_host.py builds and runs it; CPU only).
#include <stdio.h>

#include <numeric>
#include <random>

#include "ck_host.h"

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                             \
        }                                                         \
    } while (0)

int main() {
    std::mt19937_64 rng(11);
    // ---- block members: random labels, every block hit; then the faults
    const int32_t r = 37;
    const int64_t m = 5000;
    std::vector<int32_t> block((size_t)m);
    for (int64_t a = 0; a < m; ++a) block[(size_t)a] = a < r ? (int32_t)a : (int32_t)(rng() % r);
    std::vector<int> off;
    std::vector<int64_t> member;
    int64_t q_max = 0, at = -1;
    CHECK(ck_host_block_members(block.data(), m, r, off, member, &q_max, &at) == CK_HOST_BLOCKS_OK);
    CHECK((int64_t)off.size() == r + 1 && off[0] == 0 && off[(size_t)r] == m && (int64_t)member.size() == m);
    int64_t largest = 0;
    for (int32_t b = 0; b < r; ++b) {
        largest = std::max<int64_t>(largest, off[(size_t)b + 1] - off[(size_t)b]);
        for (int k = off[(size_t)b]; k < off[(size_t)b + 1]; ++k) {
            CHECK(block[(size_t)member[(size_t)k]] == b);
            CHECK(k == off[(size_t)b] || member[(size_t)k] > member[(size_t)k - 1]);
        }
    }
    CHECK(largest == q_max);
    block[77] = r;
    block[99] = -1;
    CHECK(ck_host_block_members(block.data(), m, r, off, member, &q_max, &at) == CK_HOST_BLOCKS_LABEL && at == 77);
    for (auto& x : block) x = x == 5 || x == r || x < 0 ? 6 : x;
    CHECK(ck_host_block_members(block.data(), m, r, off, member, &q_max, &at) == CK_HOST_BLOCKS_EMPTY && at == 5);
    CHECK(off[5] == off[6] && off[(size_t)r] == m);
    const int32_t one = 0;
    CHECK(ck_host_block_members(&one, 1, 1, off, member, &q_max, &at) == CK_HOST_BLOCKS_OK && q_max == 1 && member[0] == 0);
    // ---- the local layout on top of it
    {
        std::vector<double> centres(2 * (size_t)r, 1.0), xy(2 * (size_t)m, 2.0), w((size_t)m, 0.5);
        for (auto& x : block) x = x == 6 ? 5 : x;   // block 6 empty now
        CkLocalBlockLayout lay;
        CHECK(ck_host_local_block_layout(centres.data(), r, xy.data(), m, block.data(), w.data(), 64, &lay) == -1);
        block[3] = 6;
        CHECK(ck_host_local_block_layout(centres.data(), r, xy.data(), m, block.data(), w.data(), 64, &lay) == 0);
        CHECK(lay.mpad == 5056 && (int64_t)lay.xy.size() == 2 * lay.mpad && lay.perm.size() == (size_t)m);
        w[10] = NAN;
        block[20] = r;
        CHECK(ck_host_local_block_layout(centres.data(), r, xy.data(), m, block.data(), w.data(), 64, &lay) == -1);
        block[20] = 0;
        w[10] = 0.5;
    }
    // ---- prior pieces
    {
        CHECK(ck_host_block_members(block.data(), m, r, off, member, &q_max, &at) == CK_HOST_BLOCKS_OK);
        std::vector<long long> poff;
        const int64_t nd = ck_host_prior_pieces(off.data(), r, 0, poff);
        CHECK((int64_t)poff.size() == r + 1 && poff.back() == nd);
        const int64_t nf = ck_host_prior_pieces(off.data(), r, 1, poff);
        CHECK((int64_t)poff.size() == (int64_t)r * (r + 1) / 2 + 1 && poff.back() == nf && nf >= nd);
        for (size_t e = 1; e < poff.size(); ++e) CHECK(poff[e] > poff[e - 1]);
    }
    // ---- chunk rules
    CHECK(ck_host_block_chunk(0, 0, -1, 0, 1024, 100000) == CK_HOST_AUX_ALIGN);
    CHECK(ck_host_block_chunk(0, 1LL << 40, 1LL << 20, 1LL << 30, 1024, 1LL << 30) == (1LL << 30) / 8192 - CK_HOST_AUX_ALIGN);
    CHECK(ck_host_block_chunk(7, 0, -1, 0, 1024, 5) == 5);
    CHECK(ck_host_draw_chunk(0, 0, 512, 300, true, 1000) == 128);
    CHECK(ck_host_draw_chunk(0, INT64_MAX, 512, 300, false, 100000) == 8192);
    CHECK(ck_host_draw_chunk(300, 0, 512, 300, false, 200) == 200);
    // ---- coincident sites
    {
        const int64_t n = 3000;
        std::vector<double> xy(2 * (size_t)n);
        for (auto& x : xy) x = (double)(rng() % 1000000) / 7.0;
        std::vector<int> cmap((size_t)n);
        std::iota(cmap.begin(), cmap.end(), 0);
        std::shuffle(cmap.begin(), cmap.end(), rng);
        std::vector<unsigned char> mask((size_t)n, 0);
        for (int pair = 0; pair < 2; ++pair) {   // internal positions (100, 2000) and (50, 700): 700 is reported
            const int64_t a = pair == 0 ? 100 : 50, b = pair == 0 ? 2000 : 700;
            xy[2 * (size_t)cmap[(size_t)b]] = xy[2 * (size_t)cmap[(size_t)a]];
            xy[2 * (size_t)cmap[(size_t)b] + 1] = xy[2 * (size_t)cmap[(size_t)a] + 1];
        }
        CHECK(ck_host_coincident_site(xy.data(), cmap.data(), mask.data(), n) == 700);
        mask[50] = 1;
        CHECK(ck_host_coincident_site(xy.data(), cmap.data(), mask.data(), n) == 2000);
        mask[2000] = 1;
        CHECK(ck_host_coincident_site(xy.data(), cmap.data(), mask.data(), n) == -1);
        CHECK(ck_host_coincident_site(xy.data(), cmap.data(), mask.data(), 1) == -1);
    }
    // ---- the universal epilogue, large enough for the thread team, at the full trend width
    {
        const int p = CK_HOST_TREND_QMAX - 1, pi = 8, offi = 8;
        const int64_t n = 200000;
        std::vector<double> W((size_t)(n * (p + 2))), beta((size_t)p, 0.25), Ai((size_t)p * p, 0.0), f0((size_t)(n * pi), 1.0);
        for (auto& x : W) x = (double)(rng() % 1000) / 1000.0;
        for (int j = 0; j < p; ++j) Ai[(size_t)(j * p + j)] = 1.0;
        std::vector<int64_t> pperm((size_t)n);
        std::iota(pperm.begin(), pperm.end(), 0);
        std::shuffle(pperm.begin(), pperm.end(), rng);
        std::vector<double> pred((size_t)n, -1.0), err((size_t)n, -1.0);
        ck_host_universal_finish(W.data(), beta.data(), Ai.data(), f0.data(), pperm.data(), 0.5, n, p, pi, offi, pred.data(), err.data());
        for (int64_t s = 0; s < n; ++s) CHECK(err[(size_t)s] >= 0.0 && pred[(size_t)s] == pred[(size_t)s]);
        ck_host_universal_finish(W.data(), beta.data(), Ai.data(), nullptr, nullptr, -100.0, n, p, 0, 0, pred.data(), err.data());
        CHECK(ck_host_err_of(-1.0) == 0.0 && ck_host_err_of(4.0) == 2.0);
    }
    printf("all checks passed\n");
    return 0;
}
