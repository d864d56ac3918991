// TEST-ONLY shim: the plan of the local predictor (csrc/ck_host.cpp: ck_host_local_needs, ck_host_local_plan) compiled with g++,
// so that tests/test_local_plan_host.py can check it without a GPU.  Never linked into the product library.
#include "ck_host.h"

// Arrays sized by the caller for m points: need / tiled / off (m), batches / tbatches (2 m: begin, end), sys (5 m: off, k, kq, ld,
// p).  scalars[7]: k_max, n_empty, need_max, slab_doubles, tiled points, batches, tiled batches.
extern "C" void shim_local_plan(const int* cnt, long long m, int lds_limit, int k_hi, int trend, long long budget, long long* scalars,
                                long long* need, long long* tiled, long long* off, long long* batches, long long* sys,
                                long long* tbatches) {
    CkLocalNeeds nd;
    ck_host_local_needs(cnt, m, lds_limit, k_hi, trend, &nd);
    CkLocalPlan P;
    ck_host_local_plan(cnt, nd, budget, trend, &P);
    const long long sc[7] = {nd.k_max, nd.n_empty, nd.need_max, P.slab_doubles, (long long)nd.tiled.size(), (long long)P.batches.size(),
                             (long long)P.tbatches.size()};
    std::copy(sc, sc + 7, scalars);
    std::copy(nd.need.begin(), nd.need.end(), need);
    std::copy(nd.tiled.begin(), nd.tiled.end(), tiled);
    std::copy(P.off.begin(), P.off.end(), off);
    for (size_t b = 0; b < P.batches.size(); ++b) batches[2 * b] = P.batches[b].first, batches[2 * b + 1] = P.batches[b].second;
    for (size_t b = 0; b < P.tbatches.size(); ++b) tbatches[2 * b] = P.tbatches[b].first, tbatches[2 * b + 1] = P.tbatches[b].second;
    for (size_t t = 0; t < P.sys.size(); ++t) {
        const CkLocalSys& x = P.sys[t];
        const long long v[5] = {x.off, x.k, x.kq, x.ld, x.p};
        std::copy(v, v + 5, sys + 5 * t);
    }
}
