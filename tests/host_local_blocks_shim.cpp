// TEST-ONLY shim: the member layout of block cokriging in the neighbourhood (csrc/ck_host.cpp: ck_host_local_block_layout)
// compiled with g++, so that tests/test_local_blocks_host.py can check it without a GPU.  Never linked into the product library.
#include <string.h>

#include "ck_host.h"

extern "C" const char* ck_last_error(void);

// Arrays sized by the caller: off (r + 1), perm (m), xy (2 mpad), w (mpad) with mpad = m rounded up to pad; scalars[2]: mpad,
// q_max.  Returns 0, or -1 with the refusal's text in err (err_cap bytes).
extern "C" int shim_local_block_layout(const double* centres, int r, const double* pcoords, long long m, const int* block,
                                       const double* weight, int pad, long long* scalars, int* off, long long* perm, double* xy,
                                       double* w, char* err, int err_cap) {
    CkLocalBlockLayout L;
    if (ck_host_local_block_layout(centres, r, pcoords, m, block, weight, pad, &L)) {
        if (err && err_cap > 0) {
            strncpy(err, ck_last_error(), (size_t)err_cap - 1);
            err[err_cap - 1] = 0;
        }
        return -1;
    }
    scalars[0] = L.mpad;
    scalars[1] = L.q_max;
    std::copy(L.off.begin(), L.off.end(), off);
    std::copy(L.perm.begin(), L.perm.end(), perm);
    std::copy(L.xy.begin(), L.xy.end(), xy);
    std::copy(L.w.begin(), L.w.end(), w);
    return 0;
}
