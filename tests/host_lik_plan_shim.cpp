// TEST-ONLY shim: the pure planning of the dense likelihood family (csrc/ck_host.cpp: ck_host_mem_admit, ck_host_fisher_plan,
// ck_host_reml_start) compiled with g++, so that tests/test_lik_plan_host.py can check it against Python and numpy without a
// GPU.  Never linked into the product library.
#include "ck_host.h"

extern "C" int64_t shim_tri_bytes(int64_t Mp) { return ck_host_tri_bytes(Mp); }
extern "C" int64_t shim_schur_bytes(int64_t Mp) { return ck_host_schur_bytes(Mp); }

// st: free, arena (0 / 1), arena_size, arena_used, held rhs bytes, held Schur order, held slab bytes; ask: rhs bytes, Schur order,
// slab bytes, extra bytes; out: need, avail, arena_short
extern "C" void shim_mem_admit(const int64_t* st, const int64_t* ask, int64_t* out) {
    const CkMemState s = {st[0], st[1] != 0, st[2], st[3], st[4], st[5], st[6]};
    const CkMemAdmit a = ck_host_mem_admit(s, {ask[0], ask[1], ask[2], ask[3]});
    out[0] = a.need, out[1] = a.avail, out[2] = a.arena_short ? 1 : 0;
}

// geom: c0[2] wpad[2] nlo[2] nhi[2] pK0[2] npan[2]; scal: d_total b_total b_max fixed_bytes region n_units n_groups;
// units: up to 14 x (op, r, kp, d_doubles); group_of[a]: the group of operand a, -1 = in none
extern "C" int shim_fisher_plan(int n_procs, int64_t Npad, int64_t n0p, int nK, const unsigned char* op_live, int64_t room, int p,
                                int64_t ngr, int64_t cap, int64_t* geom, int64_t* b_doubles, int64_t* scal, int64_t* units,
                                int32_t* group_of) {
    bool live[CK_HOST_FISHER_NOPS];
    for (int a = 0; a < CK_HOST_FISHER_NOPS; ++a) live[a] = op_live[a] != 0;
    CkFisherPlan P;
    const int rc = ck_host_fisher_plan(n_procs, Npad, n0p, nK, live, room, p, ngr, cap, &P);
    for (int r = 0; r < 2; ++r) {
        geom[r] = P.c0[r], geom[2 + r] = P.wpad[r], geom[4 + r] = P.nlo[r], geom[6 + r] = P.nhi[r];
        geom[8 + r] = P.pK0[r], geom[10 + r] = P.npan[r];
    }
    for (int a = 0; a < CK_HOST_FISHER_NOPS; ++a) b_doubles[a] = P.b_doubles[a], group_of[a] = -1;
    scal[0] = P.d_total, scal[1] = P.b_total, scal[2] = P.b_max, scal[3] = P.fixed_bytes, scal[4] = P.region;
    scal[5] = (int64_t)P.units.size(), scal[6] = (int64_t)P.groups.size();
    for (size_t u = 0; u < P.units.size(); ++u)
        units[4 * u] = P.units[u].op, units[4 * u + 1] = P.units[u].r, units[4 * u + 2] = P.units[u].kp, units[4 * u + 3] = P.units[u].d_doubles;
    for (size_t g = 0; g < P.groups.size(); ++g)
        for (int a : P.groups[g]) group_of[a] = group_of[a] == -1 ? (int32_t)g : -2;   // -2: listed twice
    return rc;
}

extern "C" void shim_reml_start(int p, int64_t Npad, const double* W, const double* beta, const double* R, double* av) {
    ck_host_reml_start(p, Npad, W, 1 + p, beta, R, av);
}
