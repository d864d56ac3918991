// TEST-ONLY shim: the Philox4x32-10 generator and the Box-Muller normals of csrc/ck_rng.h (ck_conditional_draws) compiled
// for the host with g++, so that tests/test_host_rng.py can check them against numpy without a GPU.  Never linked into the
// product library.  With CK_SHIM_ROCRAND it also wraps rocRAND's host-callable Philox4x32-10 as an independent reference.
#include "ck_rng.h"
#if defined(CK_SHIM_ROCRAND)
#include <rocrand/rocrand_philox4x32_10.h>
// the block function is protected in rocRAND's engine
struct ShimPhilox : rocrand_device::philox4x32_10_engine {
    uint4 block(uint4 c, uint2 k) { return ten_rounds(c, k); }
};
#endif

extern "C" {
// the four output words of n (counter, key) sets: ctr 4 words and key 2 words per set
void shim_philox(const uint32_t* ctr, const uint32_t* key, long n, uint32_t* out) {
    for (long i = 0; i < n; ++i) {
        const CkPhilox4 w = ck_philox4x32_10(ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], key[2 * i], key[2 * i + 1]);
        for (int q = 0; q < 4; ++q) out[4 * i + q] = w.x[q];
    }
}
// the normals of draws 0 .. n_draws - 1 at sites 0 .. n_sites - 1 (out: n_draws x n_sites, row-major), as k_draw_noise
void shim_normals(uint64_t seed, long n_sites, long n_draws, double* out) {
    for (long k = 0; k < n_sites; ++k)
        for (long d = 0; d < n_draws; d += 2) {
            double z[2];
            ck_rng_normal2(seed, (uint32_t)k, (uint32_t)(d >> 1), z);
            out[d * n_sites + k] = z[0];
            if (d + 1 < n_draws) out[(d + 1) * n_sites + k] = z[1];
        }
}
#if defined(CK_SHIM_ROCRAND)
void shim_rocrand_philox(const uint32_t* ctr, const uint32_t* key, long n, uint32_t* out) {
    ShimPhilox e;
    for (long i = 0; i < n; ++i) {
        const uint4 c = {ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3]};
        const uint2 k = {key[2 * i], key[2 * i + 1]};
        const uint4 w = e.block(c, k);
        out[4 * i] = w.x;
        out[4 * i + 1] = w.y;
        out[4 * i + 2] = w.z;
        out[4 * i + 3] = w.w;
    }
}
#endif
}
