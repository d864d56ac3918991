// TEST-ONLY program: the radix select of csrc/ck_select.h under -fsanitize=address,undefined (tests/test_select_host.py builds
// and runs it; CPU only) on the key sets of that test, against std::nth_element.
#include <float.h>
#include <math.h>
#include <stdio.h>

#include <algorithm>
#include <random>

#include "host_select_rounds.h"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
            return 1;                                                   \
        }                                                               \
    } while (0)

static int check(const std::vector<double>& d, long rank) {
    double stat = -1.0;
    long n_le = -1;
    CHECK(host_select(d.data(), (long)d.size(), rank, &stat, &n_le) == 0);
    std::vector<double> s(d);
    std::nth_element(s.begin(), s.begin() + (rank - 1), s.end());
    const double ref = s[(size_t)(rank - 1)];
    CHECK(stat == ref && signbit(stat) == 0);
    CHECK(n_le == (long)std::count_if(d.begin(), d.end(), [&](double x) { return x <= ref; }));
    return 0;
}

static int check_ranks(const std::vector<double>& d) {
    const long n = (long)d.size();
    for (long rank : {1L, 2L, n / 2, n - 1, n})
        if (rank >= 1 && rank <= n) CHECK(check(d, rank) == 0);
    return 0;
}

int main() {
    std::mt19937_64 rng(11);
    std::uniform_real_distribution<double> U(0.0, 600.0);
    for (size_t n : {1u, 2u, 255u, 256u, 257u, 5000u}) {
        std::vector<double> d(n);
        for (auto& x : d) x = U(rng);
        CHECK(check_ranks(d) == 0);
        for (auto& x : d) x = floor(x / 50.0);   // many ties
        CHECK(check_ranks(d) == 0);
    }
    CHECK(check_ranks(std::vector<double>(300, 7.25)) == 0);   // all keys equal
    std::vector<double> two(100, 1.0);
    std::fill(two.begin() + 40, two.end(), nextafter(1.0, 2.0));   // two values one ulp apart, the rank on either side
    for (long rank : {1L, 40L, 41L, 100L}) CHECK(check(two, rank) == 0);
    const double max_dist = 0.3;
    std::vector<double> edge = {0.0, -0.0, 4.9e-324, DBL_MIN / 2, DBL_MIN, max_dist, nextafter(max_dist, 0.0), 1e-300, 0.0, max_dist};
    for (long rank = 1; rank <= (long)edge.size(); ++rank) CHECK(check(edge, rank) == 0);
    double stat;
    long n_le;
    CHECK(host_select(edge.data(), (long)edge.size(), 0, &stat, &n_le) == 1);
    CHECK(host_select(edge.data(), (long)edge.size(), (long)edge.size() + 1, &stat, &n_le) == 1);
    printf("all checks passed\n");
    return 0;
}
