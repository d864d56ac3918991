// TEST-ONLY program: the member layout of block cokriging in the neighbourhood (csrc/ck_host.cpp: ck_host_local_block_layout)
// under -fsanitize=address,undefined (tests/test_local_blocks_host.py builds and runs it; CPU only).
#include <math.h>
#include <stdio.h>
#include <string.h>

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

struct Input {
    std::vector<double> centres, pc, w;
    std::vector<int32_t> lab;
    int32_t r;
};

// the layout against its definition: offsets from the counts, a stable grouping, rows and weights gathered through perm, zeros
// in the padding
static int run(const Input& in, int pad) {
    const int64_t m = (int64_t)in.lab.size();
    CkLocalBlockLayout L;
    CHECK(ck_host_local_block_layout(in.centres.data(), in.r, in.pc.data(), m, in.lab.data(), in.w.data(), pad, &L) == 0);
    CHECK((int64_t)L.off.size() == in.r + 1 && (int64_t)L.perm.size() == m && L.off[0] == 0 && L.off[(size_t)in.r] == m);
    CHECK(L.mpad >= m && L.mpad % pad == 0 && L.mpad < m + pad);
    CHECK((int64_t)L.xy.size() == 2 * L.mpad && (int64_t)L.w.size() == L.mpad);
    std::vector<char> seen((size_t)m, 0);
    int64_t q_max = 0;
    for (int32_t b = 0; b < in.r; ++b) {
        CHECK(L.off[(size_t)b + 1] > L.off[(size_t)b]);
        q_max = std::max<int64_t>(q_max, L.off[(size_t)b + 1] - L.off[(size_t)b]);
        for (int k = L.off[(size_t)b]; k < L.off[(size_t)b + 1]; ++k) {
            const int64_t a = L.perm[(size_t)k];
            CHECK(a >= 0 && a < m && !seen[(size_t)a] && in.lab[(size_t)a] == b);
            CHECK(k == L.off[(size_t)b] || L.perm[(size_t)k - 1] < a);   // the caller's order inside a block
            seen[(size_t)a] = 1;
            CHECK(L.xy[2 * (size_t)k] == in.pc[2 * (size_t)a] && L.xy[2 * (size_t)k + 1] == in.pc[2 * (size_t)a + 1]);
            CHECK(L.w[(size_t)k] == in.w[(size_t)a]);
        }
    }
    CHECK(q_max == L.q_max);
    for (int64_t k = m; k < L.mpad; ++k) CHECK(L.xy[2 * (size_t)k] == 0.0 && L.xy[2 * (size_t)k + 1] == 0.0 && L.w[(size_t)k] == 0.0);
    return 0;
}

static int refused(const Input& in, const char* text) {
    CkLocalBlockLayout L;
    CHECK(ck_host_local_block_layout(in.centres.data(), in.r, in.pc.data(), (int64_t)in.lab.size(), in.lab.data(), in.w.data(), 64, &L) == -1);
    if (!strstr(ck_last_error(), text)) {
        printf("refusal \"%s\" does not say \"%s\"\n", ck_last_error(), text);
        return 1;
    }
    return 0;
}

static Input make(std::mt19937_64& rng, int32_t r, int64_t m, int mode) {   // mode 0: random labels (every block hit), 1: one per block
    Input in;
    in.r = r;
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    for (int32_t b = 0; b < 2 * r; ++b) in.centres.push_back(40.0 * u(rng));
    for (int64_t a = 0; a < m; ++a) {
        in.pc.push_back(40.0 * u(rng));
        in.pc.push_back(100.0 * u(rng));
        in.w.push_back(u(rng));
        in.lab.push_back(mode == 1 || a < r ? (int32_t)(a % r) : (int32_t)(rng() % (uint64_t)r));
    }
    for (int64_t a = m - 1; a > 0; --a) std::swap(in.lab[(size_t)a], in.lab[(size_t)(rng() % (uint64_t)(a + 1))]);
    return in;
}

int main() {
    std::mt19937_64 rng(11);
    for (int pad : {1, 64, 256}) {
        CHECK(run(make(rng, 1, 1, 0), pad) == 0);
        CHECK(run(make(rng, 1, 300, 0), pad) == 0);        // all sites in one block, r = 1
        CHECK(run(make(rng, 129, 129, 1), pad) == 0);      // every site its own block
        CHECK(run(make(rng, 37, 1000, 0), pad) == 0);      // m no multiple of the padding
        CHECK(run(make(rng, 64, 4096, 0), pad) == 0);      // m a multiple
    }
    for (int it = 0; it < 200; ++it) {
        const int32_t r = 1 + (int32_t)(rng() % 200);
        CHECK(run(make(rng, r, r + (int64_t)(rng() % 3000), 0), 64) == 0);
    }
    // every refusal, the offender named
    const Input good = make(rng, 5, 40, 0);
    Input bad = good;
    bad.lab[7] = 5;
    CHECK(refused(bad, "block label 5 of site 7 is outside [0, 5)") == 0);
    bad.lab[7] = -2;
    CHECK(refused(bad, "block label -2 of site 7") == 0);
    bad = good;
    for (auto& x : bad.lab)
        if (x == 3) x = 2;
    CHECK(refused(bad, "block 3 has no site") == 0);
    bad = good;
    bad.w[11] = NAN;
    CHECK(refused(bad, "weight of site 11 is not finite") == 0);
    bad = good;
    bad.w[0] = INFINITY;
    CHECK(refused(bad, "weight of site 0 is not finite (inf)") == 0);
    bad = good;
    bad.centres[2 * 4 + 1] = NAN;
    CHECK(refused(bad, "coordinate 1 of centre 4 is not finite") == 0);
    bad = good;
    bad.pc[2 * 39] = -INFINITY;
    CHECK(refused(bad, "coordinate 0 of site 39 is not finite (-inf)") == 0);
    bad = good;
    bad.r = 0;
    CHECK(refused(bad, "r must be >= 1, got 0") == 0);
    bad = good;
    bad.lab.clear();
    CHECK(refused(bad, "m must be in [1, 2^31), got 0") == 0);
    CHECK(run(good, 64) == 0);   // the refusals left nothing behind
    printf("all checks passed\n");
    return 0;
}
