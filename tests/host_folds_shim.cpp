// TEST-ONLY shim: the fold layout of leave-group-out cross-validation (csrc/ck_host.cpp: ck_host_fold_plan) compiled with g++,
// so that tests/test_cv_folds_host.py can check it without a GPU.  Never linked into the product library.
#include <string.h>

#include "ck_host.h"

extern "C" const char* ck_last_error(void);

// Returns 0 or -1 (err: the error text).  counts[6]: members, gather entries, tiles, small folds, big folds, small tiles.
// Arrays (any may be null; the caller sizes them from a first call): off (n_folds + 1), pos / cidx (members), gbase (n_folds),
// gpos (gather entries), tiles (5 per tile: c_off, a0, b0, ld, pos0), big (6 per big fold: off, s, kq, ld, gbase, fold).
extern "C" int shim_fold_plan(int i, int n_procs, long long n0, long long n1, long long n0p, const long long* perm0,
                              const long long* perm1, const int* fold0, const int* fold1, int n_folds, int fold_max,
                              long long* counts, long long* pm, int* off, int* pos, int* cidx, int* gbase, int* gpos,
                              long long* tiles, long long* big, long long* buffer_doubles, char* err, int err_cap) {
    const int64_t n[2] = {n0, n1};
    CkFoldPlan P;
    if (ck_host_fold_plan(i, n_procs, n, n0p, (const int64_t*)perm0, (const int64_t*)perm1, fold0, fold1, n_folds, fold_max, &P)) {
        if (err && err_cap > 0) {
            strncpy(err, ck_last_error(), (size_t)err_cap - 1);
            err[err_cap - 1] = 0;
        }
        return -1;
    }
    counts[0] = (long long)P.pos.size();
    counts[1] = (long long)P.gpos.size();
    counts[2] = (long long)P.tiles.size();
    counts[3] = (long long)P.small.size();
    counts[4] = (long long)P.big.size();
    counts[5] = P.n_small_tiles;
    pm[0] = P.pmin;
    pm[1] = P.pmax;
    *buffer_doubles = P.buffer_doubles;
    if (off) memcpy(off, P.off.data(), P.off.size() * 4);
    if (pos) memcpy(pos, P.pos.data(), P.pos.size() * 4);
    if (cidx) memcpy(cidx, P.cidx.data(), P.cidx.size() * 4);
    if (gbase) memcpy(gbase, P.gbase.data(), P.gbase.size() * 4);
    if (gpos) memcpy(gpos, P.gpos.data(), P.gpos.size() * 4);
    if (tiles)
        for (size_t t = 0; t < P.tiles.size(); ++t) {
            const CkFoldTile& x = P.tiles[t];
            const long long v[5] = {x.c_off, x.a0, x.b0, x.ld, x.pos0};
            memcpy(tiles + 5 * t, v, sizeof(v));
        }
    if (big)
        for (size_t y = 0; y < P.big.size(); ++y) {
            const CkFoldBig& b = P.big[y];
            const long long v[6] = {b.off, b.s, b.kq, b.ld, b.gbase, b.fold};
            memcpy(big + 6 * y, v, sizeof(v));
        }
    return 0;
}
