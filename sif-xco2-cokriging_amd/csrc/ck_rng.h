// ck_rng.h -- counter-based random numbers of the conditional simulation (ck_conditional_draws).
//
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): a 128-bit counter
// is enciphered under a 64-bit key by ten rounds of two 32 x 32 -> 64-bit multiplications, the key bumped by the Weyl
// constants between rounds.  No state: the normal of draw d at site k is a pure function of (seed, k, d), so a draw does
// not depend on how many draws a call makes, on the chunking, or on the library's internal site order.
//
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (k, d / 2, 0, 0)            k: the caller's site index, d: the draw index
//   u1 = (x0 << 21 | x1 >> 11) + 1/2) 2^-53,  u2 = (x2 << 21 | x3 >> 11) + 1/2) 2^-53    (two 53-bit uniforms in (0, 1))
//   r = sqrt(-2 log u1), t = 2 pi u2:  draw 2 j -> r cos t,  draw 2 j + 1 -> r sin t     (FP64 Box-Muller)
//
// CK_RNG_HD functions compile for the host as well, so that tests/host_rng_shim.cpp can check them against numpy.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CK_RNG_HD __host__ __device__ inline
#else
#define CK_RNG_HD static inline
#endif

struct CkPhilox4 {
    uint32_t x[4];
};

CK_RNG_HD CkPhilox4 ck_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        if (r > 0) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
    }
    CkPhilox4 o;
    o.x[0] = c0;
    o.x[1] = c1;
    o.x[2] = c2;
    o.x[3] = c3;
    return o;
}

// 53 random bits of two words -> (0, 1), never 0 or 1
CK_RNG_HD double ck_rng_u53(uint32_t hi, uint32_t lo) {
    const uint64_t a = ((uint64_t)hi << 21) | (uint64_t)(lo >> 11);
    return ((double)a + 0.5) * 1.1102230246251565e-16;   // 2^-53
}

// the two normals of the draw pair d / 2 at site k: out[0] for even d, out[1] for odd d
CK_RNG_HD void ck_rng_normal2(uint64_t seed, uint32_t site, uint32_t pair, double* out) {
    const CkPhilox4 w = ck_philox4x32_10(site, pair, 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double u1 = ck_rng_u53(w.x[0], w.x[1]);
    const double u2 = ck_rng_u53(w.x[2], w.x[3]);
    const double r = sqrt(-2.0 * log(u1));
    const double t = 6.283185307179586 * u2;
    out[0] = r * cos(t);
    out[1] = r * sin(t);
}
