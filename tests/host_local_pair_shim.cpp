// TEST-ONLY shim: the host planning of both processes in the moving neighbourhood (csrc/ck_host.cpp: ck_host_sim_order,
// ck_host_sim_ext, ck_host_local_pair_needs with ck_host_local_plan) compiled with g++, so that tests/test_local_pair_host.py
// can check it without a GPU.  Never linked into the product library.
#include <string.h>

#include "ck_host.h"

// pos: m0 + m1 ints.  0, or -1 with the two stacked sites of equal rank in dup2.
extern "C" int shim_sim_order(const long long* rank, long long m0, long long m1, int* pos, long long* dup2) {
    const int64_t m[2] = {m0, m1};
    CkSimSites S;
    const int rc = ck_host_sim_order(reinterpret_cast<const int64_t*>(rank), m, &S);
    dup2[0] = S.dup[0];
    dup2[1] = S.dup[1];
    if (rc == 0) memcpy(pos, S.pos.data(), S.pos.size() * sizeof(int));
    return rc;
}

// the augmented set's maps: perm_q has n_q + m_q entries; ext, rs: npad ints, rp: m0 + m1
extern "C" int shim_sim_ext(const long long* rank, int n_procs, long long n0, long long n1, long long m0, long long m1, long long n0p,
                            long long npad, const long long* perm0, const long long* perm1, int* ext, int* rs, int* rp) {
    const int64_t n[2] = {n0, n1}, m[2] = {m0, m1};
    CkSimSites S;
    if (ck_host_sim_order(reinterpret_cast<const int64_t*>(rank), m, &S)) return -1;
    ck_host_sim_ext(n_procs, n, m, n0p, npad, reinterpret_cast<const int64_t*>(perm0), reinterpret_cast<const int64_t*>(perm1), &S);
    memcpy(ext, S.ext.data(), S.ext.size() * sizeof(int));
    memcpy(rs, S.rs.data(), S.rs.size() * sizeof(int));
    memcpy(rp, S.rp.data(), S.rp.size() * sizeof(int));
    return 0;
}

// The size classes of ck_predict_local_pair for m neighbour counts.  cls[p]: 0 empty, 1 LDS, 2 tiled; kq / ld / off: the tiled
// system of point p (0 elsewhere); out3: slab_doubles, the number of tiled batches, need_max.
extern "C" void shim_pair_classes(const int* cnt, long long m, int lds_limit, int tile_min, long long budget, int* cls, int* kq,
                                  int* ld, long long* off, long long* out3) {
    CkLocalNeeds nd;
    ck_host_local_pair_needs(cnt, m, lds_limit, tile_min, &nd);
    CkLocalPlan plan;
    ck_host_local_plan(cnt, nd, budget < nd.need_max ? nd.need_max : budget, CK_LOCAL_PAIR_ROWS - 2, &plan);
    for (long long p = 0; p < m; ++p) {
        cls[p] = cnt[p] == 0 ? 0 : 1;
        kq[p] = ld[p] = 0;
        off[p] = 0;
    }
    for (const CkLocalSys& s : plan.sys) {
        cls[s.p] = 2;
        kq[s.p] = s.kq;
        ld[s.p] = s.ld;
        off[s.p] = s.off;
    }
    out3[0] = plan.slab_doubles;
    out3[1] = plan.sys.empty() ? 0 : (long long)plan.tbatches.size();
    out3[2] = nd.need_max;
}
