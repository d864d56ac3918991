// TEST-ONLY shim: the dense predictors' host arithmetic (csrc/ck_host.cpp: ck_host_block_members, ck_host_prior_pieces,
// ck_host_block_chunk, ck_host_draw_chunk, ck_host_coincident_site, ck_host_universal_finish) compiled with g++, so that
// tests/test_dense_predict_host.py can check it without a GPU.  Never linked into the product library.
#include <string.h>

#include "ck_host.h"

// off: r + 1, member: m.  out[2]: the largest block, the offending site or block.  Returns the fault code.
extern "C" int shim_block_members(const int* block, long long m, int r, int* off, long long* member, long long* out) {
    std::vector<int> o;
    std::vector<int64_t> mem;
    int64_t q_max = -1, at = -1;
    const int rc = ck_host_block_members(block, m, r, o, mem, &q_max, &at);
    out[0] = q_max;
    out[1] = at;
    if (rc == CK_HOST_BLOCKS_LABEL) return rc;
    memcpy(off, o.data(), o.size() * sizeof(int));
    memcpy(member, mem.data(), mem.size() * sizeof(int64_t));
    return rc;
}

// poff: r + 1 (diagonal) or r (r + 1) / 2 + 1 (full) entries.  Returns the number of pieces.
extern "C" long long shim_prior_pieces(const int* off, int r, int full, long long* poff) {
    std::vector<long long> p;
    const long long n = ck_host_prior_pieces(off, r, full, p);
    memcpy(poff, p.data(), p.size() * sizeof(long long));
    return n;
}

extern "C" long long shim_block_chunk(long long option, long long free_bytes, long long arena_rest, long long held_bytes,
                                      long long Npad, long long m) {
    return ck_host_block_chunk(option, free_bytes, arena_rest, held_bytes, Npad, m);
}

extern "C" long long shim_draw_chunk(long long option, long long free_bytes, long long Mp, long long m, int caller_noise,
                                     long long n_draws) {
    return ck_host_draw_chunk(option, free_bytes, Mp, m, caller_noise != 0, n_draws);
}

extern "C" long long shim_coincident_site(const double* pcoords, const int* cmap, const unsigned char* mask, long long m) {
    return ck_host_coincident_site(pcoords, cmap, mask, m);
}

extern "C" void shim_universal_finish(const double* W, const double* beta, const double* Ainv, const double* f0,
                                      const long long* pperm, double c0, long long m, int p, int pi, int offi, double* pred,
                                      double* pred_err) {
    ck_host_universal_finish(W, beta, Ainv, f0, (const int64_t*)pperm, c0, m, p, pi, offi, pred, pred_err);
}

extern "C" double shim_err_of(double var) { return ck_host_err_of(var); }
