// ck_select.h -- the order statistic behind the local predictor's neighbour cap (ck_set_local_neighbours): the rank-th smallest
// of n non-negative distances by an MSB-first radix select over their bit patterns, 8 rounds of 8 bits.
// Compiles for the host and for the device: k_local_select (ck_local.hip) fills the 256-bin histogram of a round with integer
// LDS atomics and one thread narrows; tests/host_select_shim.cpp drives the same rounds serially with g++ so that the logic
// can be checked against numpy without a GPU.
//
// A round looks at the keys that agree with the prefix found so far, bins them by the next 8 bits, and moves into the bin
// that holds the wanted rank.  After 8 rounds the prefix IS the order statistic, `less` the number of keys below it and
// `ties` the number of keys equal to it: less + ties keys are <= the statistic -- every tie at the cut is counted, and the
// result depends on the multiset of keys alone, not on the order they arrive in.  Integers only: no rounding anywhere.
#pragma once

#include <stdint.h>

#ifndef CK_HD   // as in ck_math.h
#if defined(__HIPCC__)
#define CK_HD __host__ __device__ __forceinline__
#else
#define CK_HD inline
#endif
#endif

#define CK_SEL_ROUNDS 8
#define CK_SEL_BINS 256

// The bit pattern of a non-negative double is monotone in its value (0.0, denormals and infinity included); -0.0 maps to 0.0
CK_HD uint64_t ck_sel_key(double d) {
    if (d == 0.0) return 0;
    union {
        double f;
        uint64_t u;
    } c;
    c.f = d;
    return c.u;
}

CK_HD double ck_sel_dist(uint64_t key) {
    union {
        double f;
        uint64_t u;
    } c;
    c.u = key;
    return c.f;
}

struct CkSelState {
    uint64_t prefix;   // the bits decided so far (the top 8 * round), zeros below
    int64_t rank;      // 1-based rank wanted among the keys that agree with the prefix
    int64_t less;      // keys below every key that agrees with the prefix
    int64_t ties;      // keys in the bin chosen last
    int round;         // rounds done
};

CK_HD void ck_sel_begin(CkSelState* s, int64_t rank) {
    s->prefix = 0;
    s->rank = rank;
    s->less = 0;
    s->ties = 0;
    s->round = 0;
}

// does the key take part in this round, and in which bin
CK_HD bool ck_sel_match(const CkSelState* s, uint64_t key) {
    return s->round == 0 || ((key ^ s->prefix) >> (64 - 8 * s->round)) == 0;
}

CK_HD int ck_sel_digit(const CkSelState* s, uint64_t key) { return (int)((key >> (56 - 8 * s->round)) & 255u); }

// hist: this round's counts of the matching keys (1 <= rank <= their total).  Every bin is read: no data-dependent exit.
CK_HD void ck_sel_narrow(CkSelState* s, const unsigned* hist) {
    int64_t cum = 0, below = 0, ties = 0;
    int digit = 0;
    for (int b = 0; b < CK_SEL_BINS; ++b) {
        const int64_t c = hist[b];
        if (cum < s->rank && cum + c >= s->rank) {
            digit = b;
            below = cum;
            ties = c;
        }
        cum += c;
    }
    s->prefix |= (uint64_t)digit << (56 - 8 * s->round);
    s->rank -= below;
    s->less += below;
    s->ties = ties;
    s->round += 1;
}
