// TEST-ONLY shim: the radix select behind the local predictor's neighbour cap (csrc/ck_select.h) compiled for the host, its
// eight rounds driven serially the way k_local_select drives them with a workgroup (tests/test_select_host.py; no GPU).
#include "host_select_rounds.h"

extern "C" {
// the rank-th smallest (1-based) of n non-negative distances and the number of them <= it; 0 on success
int shim_select(const double* d, long n, long rank, double* stat, long* n_le) { return host_select(d, n, rank, stat, n_le); }
unsigned long long shim_key(double d) { return ck_sel_key(d); }
}
