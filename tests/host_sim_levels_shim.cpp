// TEST-ONLY shim: the level planner of the local conditional simulation (csrc/ck_host.cpp: ck_host_sim_levels) compiled with
// g++, so that tests/test_local_sim_host.py can check it without a GPU.  Never linked into the product library.
#include "ck_host.h"

// Arrays sized by the caller: level / order (m ints), off (m + 1 words; on -1 its first two hold the offending site and entry).
// Returns ck_host_sim_levels' value.
extern "C" long long shim_sim_levels(long long m, int ld, const int* pos, const int* ns, const int* nbr, int* level, int* order,
                                     long long* off) {
    CkSimLevels lv;
    const int64_t n = ck_host_sim_levels(m, ld, pos, ns, nbr, &lv);
    std::copy(lv.off.begin(), lv.off.end(), off);
    if (n < 0) return n;
    std::copy(lv.level.begin(), lv.level.end(), level);
    std::copy(lv.order.begin(), lv.order.end(), order);
    return n;
}
