// TEST-ONLY: the eight rounds of csrc/ck_select.h driven serially (shared by host_select_shim.cpp and
// host_select_sanitize_main.cpp): per round the histogram of the keys that agree with the prefix, then the narrowing step.
#pragma once
#include <stddef.h>

#include <vector>

#include "ck_select.h"

static inline int host_select(const double* d, long n, long rank, double* stat, long* n_le) {
    if (n <= 0 || rank < 1 || rank > n) return 1;
    std::vector<uint64_t> keys((size_t)n);
    for (long e = 0; e < n; ++e) keys[(size_t)e] = ck_sel_key(d[e]);
    CkSelState st;
    ck_sel_begin(&st, rank);
    for (int round = 0; round < CK_SEL_ROUNDS; ++round) {
        unsigned hist[CK_SEL_BINS] = {};
        for (uint64_t key : keys)
            if (ck_sel_match(&st, key)) hist[ck_sel_digit(&st, key)] += 1;
        ck_sel_narrow(&st, hist);
    }
    *stat = ck_sel_dist(st.prefix);
    *n_le = (long)(st.less + st.ties);
    return 0;
}
