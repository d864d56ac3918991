// TEST-ONLY shim: the plan of cross-validation in the moving neighbourhood (csrc/ck_host.cpp: ck_host_local_cv_plan) compiled with
// g++, so that tests/test_local_cv_folds_host.py can check it without a GPU.  Never linked into the product library.
#include <string.h>

#include "ck_host.h"

extern "C" const char* ck_last_error(void);

// Arrays sized by the caller: plist / fp / idx (n_i), off (max(n_folds, 1) + 1), size (n_folds), gself (n0 + n1).  scalars[3]: the
// number of predicted data, of groups, of offsets written.  Returns the plan's return code; msg (cap bytes) gets ck_last_error.
extern "C" int shim_local_cv_plan(int i, int n_procs, long long n0, long long n1, long long n0p, const long long* perm0,
                                  const long long* perm1, const int* fold0, const int* fold1, int n_folds, int buffer_i, long long* scalars,
                                  int* plist, int* fp, int* idx, long long* off, long long* size, int* gself, char* msg, int cap) {
    const int64_t n[2] = {n0, n1};
    CkLocalCvPlan P;
    const int rc = ck_host_local_cv_plan("shim", i, n_procs, n, n0p, (const int64_t*)perm0, (const int64_t*)perm1, fold0, fold1, n_folds,
                                         buffer_i != 0, &P);
    if (rc) {
        strncpy(msg, ck_last_error(), (size_t)cap - 1);
        msg[cap - 1] = 0;
        return rc;
    }
    scalars[0] = (long long)P.plist.size();
    scalars[1] = P.n_groups;
    scalars[2] = (long long)P.off.size();
    std::copy(P.plist.begin(), P.plist.end(), plist);
    std::copy(P.fp.begin(), P.fp.end(), fp);
    std::copy(P.idx.begin(), P.idx.end(), idx);
    std::copy(P.off.begin(), P.off.end(), off);
    std::copy(P.size.begin(), P.size.end(), size);
    std::copy(P.gself.begin(), P.gself.end(), gself);
    return 0;
}
