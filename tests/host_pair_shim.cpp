// TEST-ONLY shim: the stacked layout of the joint prediction of both processes (csrc/ck_host.cpp: ck_host_pair_plan,
// ck_host_pair_coincident) compiled with g++, so that tests/test_pair_host.py can check it without a GPU.  Never linked into
// the product library.
#include <string.h>

#include "ck_host.h"

// out4: m0p, rows, sorted[0], sorted[1].  cmap: roundup(m0, 64) + m1 ints, row_of: m0 + m1, xy: 2 (roundup(m0, 64) + m1).
extern "C" void shim_pair_plan(const double* pc0, long long m0, const double* pc1, long long m1, int site_order, long long* out4,
                               int* cmap, long long* row_of, double* xy) {
    CkPairPlan P;
    ck_host_pair_plan(pc0, m0, pc1, m1, site_order != 0, &P);
    out4[0] = P.m0p;
    out4[1] = P.rows;
    out4[2] = P.sorted[0];
    out4[3] = P.sorted[1];
    memcpy(cmap, P.cmap.data(), P.cmap.size() * sizeof(int));
    memcpy(row_of, P.row_of.data(), P.row_of.size() * sizeof(int64_t));
    memcpy(xy, P.xy.data(), P.xy.size() * sizeof(double));
}

// mask: rows bytes in the plan's internal order
extern "C" long long shim_pair_coincident(const double* pc0, long long m0, const double* pc1, long long m1, int site_order,
                                          const unsigned char* mask) {
    CkPairPlan P;
    ck_host_pair_plan(pc0, m0, pc1, m1, site_order != 0, &P);
    return ck_host_pair_coincident(P, pc0, pc1, mask);
}
