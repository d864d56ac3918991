// TEST-ONLY shim: the index work of the Vecchia ordering (csrc/ck_host.cpp: ck_host_vecchia_order) compiled with g++, so that
// tests/test_vecchia_order_host.py can check it without a GPU.  Never linked into the product library.
#include "ck_host.h"

// Arrays sized by the caller: pos / gself (n0 + n1 ints), rs (npad ints), dup (2).  Returns ck_host_vecchia_order's status; on -1
// only dup is written.
extern "C" int shim_vecchia_order(const long long* rank, int n_procs, long long n0, long long n1, long long n0p, long long npad,
                                  const long long* perm0, const long long* perm1, int* pos, int* rs, int* gself, long long* dup) {
    const int64_t n[2] = {n0, n1};
    CkVecchiaOrder ord;
    const int rc = ck_host_vecchia_order((const int64_t*)rank, n_procs, n, n0p, npad, (const int64_t*)perm0, (const int64_t*)perm1, &ord);
    dup[0] = ord.dup[0];
    dup[1] = ord.dup[1];
    if (rc) return rc;
    std::copy(ord.pos.begin(), ord.pos.end(), pos);
    std::copy(ord.rs.begin(), ord.rs.end(), rs);
    std::copy(ord.gself.begin(), ord.gself.end(), gself);
    return 0;
}
