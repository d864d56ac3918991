// ck_host.cpp -- see ck_host.h.  Nothing in this file touches the GPU.
#include "ck_host.h"
#include "ck_tilemap.h"

#include <math.h>
#include <cmath>
#include <string.h>

#include <atomic>
#include <memory>
#include <utility>

#include "../../include/cokrige.h"

#define CK_HOST_DEG2RAD 0.017453292519943295   // numpy.radians' factor pi / 180 (== CK_DEG2RAD, ck_math.h)
#define CK_HOST_EARTH_RADIUS_KM 6371.0         // == CK_EARTH_RADIUS_KM

static thread_local std::string g_err;
int ck_fail(const std::string& msg) {
    g_err = msg;
    return -1;
}
extern "C" const char* ck_last_error(void) { return g_err.c_str(); }

int ck_host_parallel_threads(int64_t n) {
    const unsigned hw = std::thread::hardware_concurrency();
    return n < 100000 ? 1 : (int)std::max(1u, std::min(8u, hw ? hw : 1u));
}

// Position along the Hilbert curve of order 16 through the unit square (x, y in [0, 65536)).  The textbook loop -- per level:
// digit (3 rx) ^ ry; if ry == 0, complement the lower bits of both coordinates when rx == 1 and exchange them -- keeps nothing but
// "exchanged" and "complemented" from level to level (the two commute), so four levels at a time come from a table indexed by
// that state and a nibble of each coordinate: 4 look-ups per point instead of 16 dependent iterations (the prediction sites of
// every ck_aux_begin are ordered on the host: 10 000 points 0.54 -> 0.1 ms).
struct HilbertTable {
    uint16_t t[4 * 256];   // [state][x nibble][y nibble] -> (8 bits of the key) << 2 | next state;  state = exchanged | complemented << 1
    HilbertTable() {
        for (unsigned st = 0; st < 4; ++st)
            for (unsigned xn = 0; xn < 16; ++xn)
                for (unsigned yn = 0; yn < 16; ++yn) {
                    unsigned sw = st & 1, cp = st >> 1, d = 0;
                    for (int b = 3; b >= 0; --b) {
                        const unsigned bx = (xn >> b) & 1, by = (yn >> b) & 1;
                        const unsigned rx = (sw ? by : bx) ^ cp, ry = (sw ? bx : by) ^ cp;
                        d = d << 2 | ((3u * rx) ^ ry);
                        if (ry == 0) {
                            if (rx == 1) cp ^= 1;
                            sw ^= 1;
                        }
                    }
                    t[st << 8 | xn << 4 | yn] = (uint16_t)(d << 2 | cp << 1 | sw);
                }
    }
};
static const HilbertTable g_hilbert;

static uint64_t hilbert_key(uint32_t x, uint32_t y) {
    uint64_t d = 0;
    unsigned st = 0;
    for (int sh = 12; sh >= 0; sh -= 4) {
        const unsigned e = g_hilbert.t[st << 8 | ((x >> sh) & 15u) << 4 | ((y >> sh) & 15u)];
        d = d << 8 | (e >> 2);
        st = e & 3u;
    }
    return d;
}

void ck_host_hilbert_order(const double* xy, int64_t n, const double lo[2], const double hi[2], std::vector<int64_t>& perm) {
    const double sx = hi[0] > lo[0] ? 65536.0 / (hi[0] - lo[0]) : 0.0, sy = hi[1] > lo[1] ? 65536.0 / (hi[1] - lo[1]) : 0.0;
    auto key_of = [&](int64_t k) -> uint32_t {   // order-16 curve: the key fits 32 bits
        double fx = (xy[2 * k] - lo[0]) * sx, fy = (xy[2 * k + 1] - lo[1]) * sy;
        fx = fx >= 0.0 ? (fx < 65535.0 ? fx : 65535.0) : 0.0;   // also catches NaN
        fy = fy >= 0.0 ? (fy < 65535.0 ? fy : 65535.0) : 0.0;
        return (uint32_t)hilbert_key((uint32_t)fx, (uint32_t)fy);
    };
    perm.resize((size_t)n);
    if (n < 4096) {
        std::vector<std::pair<uint32_t, int64_t>> key((size_t)n);
        for (int64_t k = 0; k < n; ++k) key[(size_t)k] = {key_of(k), k};
        std::stable_sort(key.begin(), key.end(),
                         [](const std::pair<uint32_t, int64_t>& a, const std::pair<uint32_t, int64_t>& b) { return a.first < b.first; });
        for (int64_t k = 0; k < n; ++k) perm[(size_t)k] = key[(size_t)k].second;
        return;
    }
    // large sets (a million soundings of a variogram): a stable LSD radix sort of (key, index) in three 11-bit passes
    // on a few threads -- every thread counts and scatters its own contiguous piece, the pieces' bucket offsets are laid
    // out thread after thread, so equal keys keep the caller's order.  One team of threads runs all the phases (a
    // spinning barrier in between; spawning a team per phase cost more than the phases), on uninitialised buffers
    // first touched by the threads that use them.  Per million points: comparison sort 270 ms, two 16-bit passes on one
    // thread 13 ms; with this sort, the bounding box and the gather on the same threads ck_vario_begin as a whole went
    // from 23 to 10.5 ms.
    const int nt = ck_host_parallel_threads(n);
    const int NBK = 2048;
    std::unique_ptr<uint32_t[]> buf(new uint32_t[(size_t)4 * (size_t)n]);
    uint32_t *ka = buf.get(), *kb = ka + n, *ia = kb + n, *ib = ia + n;
    std::vector<int64_t> hist((size_t)nt * NBK);
    std::atomic<int> arrived{0}, generation{0};
    auto barrier = [&]() {
        const int g = generation.load(std::memory_order_acquire);
        if (arrived.fetch_add(1, std::memory_order_acq_rel) + 1 == nt) {
            arrived.store(0, std::memory_order_relaxed);
            generation.fetch_add(1, std::memory_order_acq_rel);
        } else {
            while (generation.load(std::memory_order_acquire) == g) std::this_thread::yield();
        }
    };
    auto work = [&](int t) {
        const int64_t b = n * t / nt, e = n * (t + 1) / nt;
        int64_t* hh = &hist[(size_t)t * NBK];
        uint32_t *sk = ka, *si = ia, *dk = kb, *di = ib;
        for (int64_t k = b; k < e; ++k) {
            sk[k] = key_of(k);
            si[k] = (uint32_t)k;
        }
        for (int pass = 0; pass < 3; ++pass) {
            const int sh = 11 * pass;
            for (int bk = 0; bk < NBK; ++bk) hh[bk] = 0;
            for (int64_t k = b; k < e; ++k) ++hh[(sk[k] >> sh) & (NBK - 1)];
            barrier();
            if (t == 0) {
                int64_t run = 0;
                for (int bk = 0; bk < NBK; ++bk)
                    for (int q = 0; q < nt; ++q) {
                        const int64_t c = hist[(size_t)q * NBK + bk];
                        hist[(size_t)q * NBK + bk] = run;
                        run += c;
                    }
            }
            barrier();
            for (int64_t k = b; k < e; ++k) {
                const int64_t p = hh[(sk[k] >> sh) & (NBK - 1)]++;
                dk[p] = sk[k];
                di[p] = si[k];
            }
            barrier();
            std::swap(sk, dk);
            std::swap(si, di);
        }
        for (int64_t k = b; k < e; ++k) perm[(size_t)k] = (int64_t)si[k];
    };
    if (nt == 1) {
        work(0);
    } else {
        std::vector<std::thread> th;
        for (int t = 1; t < nt; ++t) th.emplace_back(work, t);
        work(0);
        for (auto& x : th) x.join();
    }
}

void ck_host_bounding_box(const double* xy, int64_t n, double lo[2], double hi[2]) {
    const int nt = ck_host_parallel_threads(n);
    std::vector<double> part((size_t)nt * 4);
    ck_host_parallel(n, [&](int t, int64_t b, int64_t e) {
        double l0 = 1e300, l1 = 1e300, h0 = -1e300, h1 = -1e300;
        for (int64_t k = b; k < e; ++k) {   // comparisons, not fmin / fmax (library calls: 12 ns per point); a NaN is skipped either way
            const double x = xy[2 * k], y = xy[2 * k + 1];
            l0 = x < l0 ? x : l0;
            h0 = x > h0 ? x : h0;
            l1 = y < l1 ? y : l1;
            h1 = y > h1 ? y : h1;
        }
        part[(size_t)t * 4] = l0;
        part[(size_t)t * 4 + 1] = l1;
        part[(size_t)t * 4 + 2] = h0;
        part[(size_t)t * 4 + 3] = h1;
    });
    for (int t = 0; t < nt; ++t) {
        lo[0] = fmin(lo[0], part[(size_t)t * 4]);
        lo[1] = fmin(lo[1], part[(size_t)t * 4 + 1]);
        hi[0] = fmax(hi[0], part[(size_t)t * 4 + 2]);
        hi[1] = fmax(hi[1], part[(size_t)t * 4 + 3]);
    }
}

// sklearn's haversine_distances (Cython on libm's sin / cos / asin / sqrt) of np.radians(X) times 6371, or scipy's
// cdist.  The variogram kernels leave every pair whose bin or retention they cannot decide beyond rounding to this
// function (tests/test_ref_distance.py checks it against sklearn / scipy bit by bit on the CPU).  No contraction of
// a * b + c into an fma: the reference's binaries have none.
#if defined(__clang__)
double ck_host_ref_distance(int metric, const double* a, const double* b) {
#pragma clang fp contract(off)
#else
__attribute__((optimize("fp-contract=off"))) double ck_host_ref_distance(int metric, const double* a, const double* b) {
#endif
    if (metric == CK_HOST_METRIC_EUCLID) {
        const double d0 = a[0] - b[0], d1 = a[1] - b[1];
        const double s0 = d0 * d0;
        const double s1 = d1 * d1;
        return sqrt(s0 + s1);
    }
    const double lat1 = a[0] * CK_HOST_DEG2RAD, lon1 = a[1] * CK_HOST_DEG2RAD, lat2 = b[0] * CK_HOST_DEG2RAD,
                 lon2 = b[1] * CK_HOST_DEG2RAD;
    const double sin_0 = sin(0.5 * (lat1 - lat2));
    const double sin_1 = sin(0.5 * (lon1 - lon2));
    const double c = cos(lat1) * cos(lat2) * sin_1 * sin_1;
    const double r = sin_0 * sin_0 + c;
    const double d = 2 * asin(sqrt(r));
    return d * CK_HOST_EARTH_RADIUS_KM;
}

extern "C" int ck_hilbert_order(const double* coords, int64_t n, int64_t* perm_out) {
    if (n < 0 || (n > 0 && (!coords || !perm_out))) return ck_fail("bad arguments");
    if (n >= (1LL << 32)) return ck_fail("at most 2^32 - 1 sites");
    if (n == 0) return 0;
    double lo[2] = {1e300, 1e300}, hi[2] = {-1e300, -1e300};
    ck_host_bounding_box(coords, n, lo, hi);
    std::vector<int64_t> perm;
    ck_host_hilbert_order(coords, n, lo, hi, perm);
    memcpy(perm_out, perm.data(), (size_t)n * sizeof(int64_t));
    return 0;
}

// host-only: the tiles of one Cholesky trailing update in launch order (ck_tilemap.h; tests/test_tilemap.py)
extern "C" int64_t ck_debug_tile_map(int64_t nvalid, int J0, int Jstep, int nJ, int32_t* out3, int64_t cap) {
    if (nvalid <= 0 || J0 < 0 || Jstep < 1 || nJ < 0) return ck_fail("bad arguments");
    if (4LL * J0 >= (nvalid + 127) / 128) return ck_fail("block column J0 lies in the padding");
    const CkTileMap m = ck_tilemap_make(nvalid, J0, Jstep, nJ);
    if (out3)
        for (int64_t t = 0; t < m.total && t < cap; ++t) {
            int u, tm, tn;
            ck_tilemap_get(m, t, u, tm, tn);
            out3[3 * t] = J0 + u * Jstep;
            out3[3 * t + 1] = tm;
            out3[3 * t + 2] = tn;
        }
    return m.total;
}

// host-only: the same for a "tall" launch (k_tall_group_d): every block column's triangle tiles are followed by the
// aux_tile_rows x 4 tiles of the right-hand-side block below it; out4 = (block column, tile row, tile column, 1 if the
// tile belongs to the right-hand-side block)
extern "C" int64_t ck_debug_tall_map(int64_t nvalid, int J0, int nJ, int aux_tile_rows, int32_t* out4, int64_t cap) {
    if (nvalid <= 0 || J0 < 0 || nJ < 0 || aux_tile_rows < 0) return ck_fail("bad arguments");
    if (4LL * J0 >= (nvalid + 127) / 128) return ck_fail("block column J0 lies in the padding");
    const CkTileMap m = ck_tilemap_make(nvalid, J0, 1, nJ, aux_tile_rows);
    if (out4)
        for (int64_t t = 0; t < m.total && t < cap; ++t) {
            int u, tm, tn;
            const bool ax = ck_tilemap_get(m, t, u, tm, tn);
            out4[4 * t] = J0 + u;
            out4[4 * t + 1] = tm;
            out4[4 * t + 2] = tn;
            out4[4 * t + 3] = ax ? 1 : 0;
        }
    return m.total;
}

// host-only: workgroup -> (system, unit) of a batched launch over systems with counts[y] units each (ck_tilemap.h)
extern "C" int64_t ck_debug_run_map(const int32_t* counts, int n_sys, int32_t* out2, int64_t cap) {
    if (n_sys < 0 || (n_sys > 0 && !counts)) return ck_fail("bad arguments");
    for (int y = 1; y < n_sys; ++y)
        if (counts[y] > counts[y - 1]) return ck_fail("counts must not increase");
    const CkRunMap m = ck_runmap_make(n_sys, [&](int y) { return (int)counts[y]; });
    const int64_t total = m.nruns ? m.off[m.nruns] : 0;
    if (out2)
        for (int64_t b = 0; b < total && b < cap; ++b) {
            int y, t;
            const bool real = ck_runmap_get(m, (int)b, y, t);
            out2[2 * b] = real ? y : -1;
            out2[2 * b + 1] = t;
        }
    return total;
}

extern "C" int ck_ref_distance(int metric, const double* A, const double* B, int64_t n, double* out) {
    if (metric != CK_HOST_METRIC_HAVERSINE && metric != CK_HOST_METRIC_EUCLID) return ck_fail("unknown metric");
    if (n > 0 && (!A || !B || !out)) return ck_fail("null array");
    for (int64_t k = 0; k < n; ++k) out[k] = ck_host_ref_distance(metric, A + 2 * k, B + 2 * k);
    return 0;
}

double ck_host_vario_q_of_dist(int metric, double d) {
    if (!(d >= 0.0)) return 0.0;
    if (metric == CK_HOST_METRIC_EUCLID) return d * d;
    const long double a = (long double)d / (2.0L * CK_HOST_EARTH_RADIUS_KM);
    if (a >= 1.57079632679489661923L) return 4.0 + 1e-9;   // beyond half the circumference: everything
    const long double sn = sinl(a);
    return (double)(4.0L * sn * sn);
}

// Haversine: the unit vectors carry ~1e-16 absolute error per component, so q = |u_i - u_j|^2 carries ~2 sqrt(q) 3e-16
// (measured 5e-16 sqrt(q) over lattice pairs from 5 km to 6 000 km), and the reference's own d a few ulp; Euclid: a few ulp.
double ck_host_vario_band(int metric, double q) {
    return metric == CK_HOST_METRIC_HAVERSINE ? 6e-15 * sqrt(q) + 8e-15 * q : 8e-15 * q;
}

double ck_host_vario_cmax(double qlim) {
    const double m = sqrt(qlim) * (1.0 + 1e-9) + 1e-12;
    return m == m ? m : INFINITY;
}

int ck_host_vario_levels(int metric, double max_dist, const double* edges, int nb, CkVarioLevels* lv) {
    // Levels 1 .. E in ascending order: the inner edges below the cap, then the cap.  A pair's bin is the number of
    // levels it passes (d > threshold: pd.cut's right-closed intervals, src/fields.py:214-216); a pair that passes
    // level E is not retained (d > max_dist, :212, or beyond the last edge, where pd.cut yields no bin).
    const double dcap = fmin(max_dist, edges[nb]);
    double xa[CK_HOST_VG_MAXBINS + 2], xb[CK_HOST_VG_MAXBINS + 2], tq[CK_HOST_VG_MAXBINS + 2];
    double* dthr = lv->dthr;
    int E = 0;
    for (int e = 1; e < nb && edges[e] < dcap; ++e) dthr[++E] = edges[e];
    dthr[++E] = dcap;
    dthr[0] = xa[0] = xb[0] = tq[0] = 0.0;
    lv->q_reach = 0.0;
    for (int e = 1; e <= E; ++e) {
        tq[e] = ck_host_vario_q_of_dist(metric, dthr[e]);
        if (!(tq[e] > 0.0)) return ck_fail("variogram bin edge too close to zero");
        // the binning kernel's monotone x (ck_vario.hip): Euclid x = q; haversine x = q / 2 - 1 from a dot product,
        // which costs an absolute 1e-15 of q near x = -1 on top of the band of the difference form
        const double bnd = ck_host_vario_band(metric, tq[e]) + (metric == CK_HOST_METRIC_HAVERSINE ? 3e-15 : 0.0);
        const double qa = tq[e] + bnd, qb = tq[e] - bnd;
        if (metric == CK_HOST_METRIC_HAVERSINE) {
            xa[e] = (double)(0.5L * (long double)qa - 1.0L);
            xb[e] = (double)(0.5L * (long double)qb - 1.0L);
        } else {
            xa[e] = qa;
            xb[e] = qb;
        }
        if (!(xb[e] < xa[e])) return ck_fail("variogram bin edge below the resolution of the distances");
        lv->q_reach = qa;
    }
    // Levels whose bands overlap (bins narrower than the rounding of the distances: max_dist equal to the smallest lattice
    // distance makes linspace(lo, hi) a few 1e-15 wide, and the reference then bins by the last bits of its distances)
    // form ONE level for the device, with the union of their bands; every pair inside it goes to the host, which walks
    // it up through the cluster's edges with the reference's distance.  Device bin k = passed k clusters = real bin
    // clast[k].  A cluster of one level is the ordinary case.
    int EC = 0;
    lv->cfirst[0] = lv->clast[0] = 0;
    lv->cxa[0] = lv->cxb[0] = lv->cthr[0] = 0.0;
    for (int e = 1; e <= E; ++e) {
        if (EC >= 1 && !(xb[e] > lv->cxa[EC])) {   // overlaps the cluster so far
            lv->clast[EC] = e;
            lv->cxa[EC] = xa[e];
            lv->cthr[EC] = -1.0;   // not a single threshold: the device lists the pair also for the Euclidean metric
        } else {
            ++EC;
            lv->cfirst[EC] = lv->clast[EC] = e;
            lv->cxa[EC] = xa[e];
            lv->cxb[EC] = xb[e];
            lv->cthr[EC] = dthr[e];
        }
    }
    lv->E = E;
    lv->EC = EC;
    return 0;
}

void ck_host_vario_decide_extent(int metric, const double* ci, const double* cj, const CkVarioPair* cand, int64_t nc,
                                 double max_dist, double* best_lo, double* best_hi) {
    double tlo[8], thi[8];
    for (int t = 0; t < 8; ++t) {
        tlo[t] = INFINITY;
        thi[t] = -1.0;
    }
    ck_host_parallel(nc, [&](int t, int64_t a, int64_t b) {
        double l = INFINITY, u = -1.0;
        for (int64_t k = a; k < b; ++k) {
            const double d = ck_host_ref_distance(metric, &ci[2 * (size_t)cand[k].i], &cj[2 * (size_t)cand[k].j]);
            if (d <= max_dist) {               // src/fields.py:212
                if (d > u) u = d;              // :395
                if (d > 0.0 && d < l) l = d;   // :394
            }
        }
        tlo[t] = l;
        thi[t] = u;
    });
    for (int t = 0; t < 8; ++t) {
        if (thi[t] > *best_hi) *best_hi = thi[t];
        if (tlo[t] < *best_lo) *best_lo = tlo[t];
    }
}

void ck_host_vario_fix(int metric, const double* ci, const double* cj, const double* vi, const double* vj,
                       const CkVarioPair* fix, int64_t nf, const CkVarioLevels& lv, int covariogram, double* sm,
                       long long* cnt) {
    if (nf <= 0) return;
    const int NB1 = CK_HOST_VG_MAXBINS + 1;
    std::vector<double> dsum((size_t)8 * NB1, 0.0);
    std::vector<long long> dcnt((size_t)8 * NB1, 0);
    ck_host_parallel(nf, [&](int t, int64_t a, int64_t b) {
        double* ds = &dsum[(size_t)t * NB1];
        long long* dc = &dcnt[(size_t)t * NB1];
        for (int64_t k = a; k < b; ++k) {
            const CkVarioPair& p = fix[(size_t)k];
            if (p.lev < 1 || p.lev > lv.EC) continue;
            const double d = ck_host_ref_distance(metric, &ci[2 * (size_t)p.i], &cj[2 * (size_t)p.j]);
            const int from = lv.clast[p.lev - 1];   // where the device put it: below the cluster
            int to = from;
            for (int e = lv.cfirst[p.lev]; e <= lv.clast[p.lev] && d > lv.dthr[e]; ++e) to = e;
            if (to == from) continue;
            const double va = vi[(size_t)p.i], vb = vj[(size_t)p.j];
            const double cl = covariogram ? va * vb : 0.5 * ((va - vb) * (va - vb));   // src/fields.py:382-385
            ds[from] -= cl;
            dc[from] -= 1;
            if (to < lv.E) {   // above the cap: not retained
                ds[to] += cl;
                dc[to] += 1;
            }
        }
    });
    for (int t = 0; t < 8; ++t)
        for (int b = 0; b <= lv.E && b < NB1; ++b) {
            sm[b] += dsum[(size_t)t * NB1 + b];
            cnt[b] += dcnt[(size_t)t * NB1 + b];
        }
}

// ---------------------------------------------------------------------------------------
// universal cokriging: the p x p GLS step (p <= 16; plain loops in a fixed order)
// ---------------------------------------------------------------------------------------
int ck_host_gls(int p, const double* A, const double* b, double tol, double* R_out, double* beta, double* Ainv,
                double* logdet, double* bAb) {
    if (p <= 0) {
        if (logdet) *logdet = 0.0;
        if (bAb) *bAb = 0.0;
        return 0;
    }
    std::vector<double> R((size_t)p * p, 0.0), Ri((size_t)p * p, 0.0), w((size_t)p, 0.0);
    double ld = 0.0;
    for (int j = 0; j < p; ++j) {
        const double ajj = A[(size_t)j * p + j];
        double d = ajj;
        for (int k = 0; k < j; ++k) d -= R[(size_t)j * p + k] * R[(size_t)j * p + k];
        if (!(ajj > 0.0) || !(d > tol * ajj) || !std::isfinite(d)) return j + 1;
        const double rjj = sqrt(d);
        R[(size_t)j * p + j] = rjj;
        ld += log(rjj);
        for (int i = j + 1; i < p; ++i) {
            double s = A[(size_t)i * p + j];
            for (int k = 0; k < j; ++k) s -= R[(size_t)i * p + k] * R[(size_t)j * p + k];
            R[(size_t)i * p + j] = s / rjj;
        }
    }
    // Ri = R^-1 (lower), w = R^-1 b
    for (int j = 0; j < p; ++j) {
        Ri[(size_t)j * p + j] = 1.0 / R[(size_t)j * p + j];
        for (int i = j + 1; i < p; ++i) {
            double s = 0.0;
            for (int k = j; k < i; ++k) s += R[(size_t)i * p + k] * Ri[(size_t)k * p + j];
            Ri[(size_t)i * p + j] = -s / R[(size_t)i * p + i];
        }
    }
    double q = 0.0;
    for (int i = 0; i < p; ++i) {
        double s = 0.0;
        for (int k = 0; k <= i; ++k) s += Ri[(size_t)i * p + k] * b[k];
        w[(size_t)i] = s;
        q += s * s;
    }
    if (R_out) memcpy(R_out, R.data(), (size_t)p * p * 8);
    if (Ainv || beta) {
        std::vector<double> Ai((size_t)p * p);
        for (int i = 0; i < p; ++i)   // A^-1 = R^-T R^-1: (A^-1)_il = sum_{k >= max(i, l)} Ri_ki Ri_kl
            for (int l = 0; l <= i; ++l) {
                double s = 0.0;
                for (int k = i; k < p; ++k) s += Ri[(size_t)k * p + i] * Ri[(size_t)k * p + l];
                Ai[(size_t)i * p + l] = Ai[(size_t)l * p + i] = s;
            }
        if (Ainv) memcpy(Ainv, Ai.data(), (size_t)p * p * 8);
        if (beta)   // beta = R^-T w
            for (int i = 0; i < p; ++i) {
                double s = 0.0;
                for (int k = i; k < p; ++k) s += Ri[(size_t)k * p + i] * w[(size_t)k];
                beta[i] = s;
            }
    }
    if (logdet) *logdet = 2.0 * ld;
    if (bAb) *bAb = q;
    return 0;
}

// ---------------------------------------------------------------------------------------
// Fisher information (ck_loglik_fisher): the operands' information -> the parameters'; the REML correction
// ---------------------------------------------------------------------------------------
void ck_host_fisher_coef(int n_procs, double sig1, double sig2, double rho, double* C) {
    const int NP = CK_HOST_FISHER_NPAR, NO = CK_HOST_FISHER_NOPS;
    for (int k = 0; k < NP * NO; ++k) C[k] = 0.0;
    auto c = [&](int par, int op) -> double& { return C[par * NO + op]; };
    if (n_procs == 1) {   // sigma nu len nugget | s_0
        c(0, 0) = 2.0 * sig1;
        c(1, 1) = 1.0;
        c(2, 2) = 1.0;
        c(3, 3) = 1.0;
        c(11, 11) = 1.0;
        return;
    }
    // sigma_11 sigma_22 nu_11 nu_12 nu_22 len_11 len_12 len_22 nugget_11 nugget_22 rho_12 | s_0 s_1
    c(0, 0) = 2.0 * sig1, c(0, 8) = rho * sig2;
    c(1, 4) = 2.0 * sig2, c(1, 8) = rho * sig1;
    c(2, 1) = 1.0, c(3, 9) = 1.0, c(4, 5) = 1.0;
    c(5, 2) = 1.0, c(6, 10) = 1.0, c(7, 6) = 1.0;
    c(8, 3) = 1.0, c(9, 7) = 1.0;
    c(10, 8) = sig1 * sig2;
    c(11, 11) = 1.0, c(12, 12) = 1.0;
}

void ck_host_fisher_combine(const double* C, const double* T, const unsigned char* live, double* I) {
    const int NP = CK_HOST_FISHER_NPAR, NO = CK_HOST_FISHER_NOPS;
    for (int k = 0; k < NP * NP; ++k) I[k] = 0.0;
    for (int j = 0; j < NP; ++j) {
        if (!live[j]) continue;
        for (int k = j; k < NP; ++k) {
            if (!live[k]) continue;
            double s = 0.0;
            for (int a = 0; a < NO; ++a) {
                if (C[j * NO + a] == 0.0) continue;
                for (int b = 0; b < NO; ++b)
                    if (C[k * NO + b] != 0.0) s += C[j * NO + a] * C[k * NO + b] * T[(a <= b ? a * NO + b : b * NO + a)];
            }
            I[j * NP + k] = I[k * NP + j] = s;
        }
    }
}

int ck_host_fisher_reml(int p, int nops, const double* A, const double* K, int64_t ldk, const double* Gm, double* T) {
    if (p <= 0) return 0;
    std::vector<double> Ai((size_t)p * p), zero((size_t)p, 0.0), W((size_t)nops * p * p);
    const int bad = ck_host_gls(p, A, zero.data(), 0.0, nullptr, nullptr, Ai.data(), nullptr, nullptr);
    if (bad) return bad;
    for (int a = 0; a < nops; ++a)   // W_a = A^-1 (Y_a^T H)
        for (int i = 0; i < p; ++i)
            for (int j = 0; j < p; ++j) {
                double s = 0.0;
                for (int l = 0; l < p; ++l) s += Ai[(size_t)i * p + l] * Gm[((size_t)a * p + l) * p + j];
                W[((size_t)a * p + i) * p + j] = s;
            }
    for (int a = 0; a < nops; ++a)
        for (int b = a; b < nops; ++b) {
            double t1 = 0.0, t2 = 0.0;
            for (int i = 0; i < p; ++i)
                for (int j = 0; j < p; ++j) {
                    t1 += Ai[(size_t)i * p + j] * (K[((size_t)b * p + j) * ldk + (size_t)a * p + i] + K[((size_t)a * p + j) * ldk + (size_t)b * p + i]);
                    t2 += W[((size_t)a * p + i) * p + j] * W[((size_t)b * p + j) * p + i];
                }
            const double v = T[a * nops + b] - 0.5 * t1 + 0.5 * t2;
            T[a * nops + b] = T[b * nops + a] = v;
        }
    return 0;
}

int ck_host_fisher_plan(int n_procs, int64_t Npad, int64_t n0p, int nK, const bool* op_live, int64_t room, int p, int64_t ngr,
                        int64_t cap, CkFisherPlan* out) {
    const int64_t NB = CK_HOST_NB, Np = Npad, YR = CK_HOST_FISHER_YROWS;
    CkFisherPlan& P = *out;
    P = CkFisherPlan();
    for (int r = 0; r < 2; ++r) P.c0[r] = P.wpad[r] = P.nlo[r] = P.nhi[r] = 0, P.pK0[r] = P.npan[r] = 0;
    P.wpad[0] = P.nhi[0] = Np, P.npan[0] = nK;
    if (n_procs == 2) {
        P.wpad[0] = (n0p + 127) / 128 * 128, P.nhi[0] = n0p, P.npan[0] = (int)((n0p + NB - 1) / NB);
        P.c0[1] = n0p / 128 * 128, P.wpad[1] = Np - P.c0[1], P.nlo[1] = n0p, P.nhi[1] = Np;
        P.pK0[1] = (int)(n0p / NB), P.npan[1] = nK - P.pK0[1];
    }
    for (int a = 0; a < CK_HOST_FISHER_NOPS; ++a) P.b_doubles[a] = 0;
    for (int a = 0; a < CK_HOST_FOP_DIAG0; ++a) {
        if (!op_live[a]) continue;
        if (a < CK_HOST_FOP_R01) {
            const int r = a < CK_HOST_FOP_R11 ? 0 : 1;
            P.units.push_back({a, r, r, (int64_t)P.npan[r] * P.wpad[r] * NB});
            P.b_doubles[a] = Np * P.wpad[r];
        } else {
            P.units.push_back({a, 0, 1, (int64_t)P.npan[1] * P.wpad[0] * NB});
            P.units.push_back({a, 1, 0, (int64_t)P.npan[0] * P.wpad[1] * NB});
            P.b_doubles[a] = Np * Np;
        }
        P.b_total += P.b_doubles[a];
        P.b_max = std::max(P.b_max, P.b_doubles[a]);
    }
    for (const auto& u : P.units) P.d_total += u.d_doubles;
    const int64_t thin = p > 0 ? (int64_t)nK * YR * NB + Np * YR + Np * p + YR * (YR + p) : 0;
    const int64_t npair = CK_HOST_FISHER_NOPS * (CK_HOST_FISHER_NOPS + 1) / 2;
    P.fixed_bytes = (Np * Np + P.d_total + thin + ngr * npair + 2 * Np) * 8 + (1 << 20);
    room -= P.fixed_bytes;
    if (cap > 0 && room > 0) room = std::min(room, cap);
    P.region = P.b_total;
    P.groups.assign(1, {});
    if (P.b_total * 8 <= room) {
        for (int a = 0; a < CK_HOST_FOP_DIAG0; ++a)
            if (op_live[a]) P.groups.back().push_back(a);
        return 0;
    }
    P.region = room / 16;   // two regions of products, doubles each
    if (room < 0 || P.b_max > P.region) {
        P.region = 0;
        P.groups.clear();
        return 1;
    }
    int64_t used = 0, big = 0;
    for (int a = 0; a < CK_HOST_FOP_DIAG0; ++a) {
        if (!op_live[a]) continue;
        if (used + P.b_doubles[a] > P.region && !P.groups.back().empty()) {
            P.groups.emplace_back();
            used = 0;
        }
        P.groups.back().push_back(a);
        used += P.b_doubles[a];
        big = std::max(big, used);
    }
    P.region = big;
    return 0;
}

// ---------------------------------------------------------------------------------------
// REML: the rank-(1 + p) start of G from the reduced unit rows
// ---------------------------------------------------------------------------------------
void ck_host_reml_start(int p, int64_t Npad, const double* W, int q, const double* beta, const double* R, double* av) {
    for (int64_t r = 0; r < Npad; ++r) {
        const double* wr = &W[(size_t)((q + r) * (q + 1))];   // unit row of internal position r
        double a = wr[1];
        for (int j = 0; j < p; ++j) a -= wr[2 + j] * beta[j];
        av[(size_t)r] = a;
        for (int j = 0; j < p; ++j) {   // C_r = R^-1 B_r (forward substitution)
            double c = wr[2 + j];
            for (int l = 0; l < j; ++l) c -= R[(size_t)(j * p + l)] * av[(size_t)(1 + l) * Npad + r];
            av[(size_t)(1 + j) * Npad + r] = c / R[(size_t)(j * p + j)];
        }
    }
}

// ---------------------------------------------------------------------------------------
// device memory admission: free memory plus what the call releases first, against what it must take
// ---------------------------------------------------------------------------------------
CkMemAdmit ck_host_mem_admit(const CkMemState& st, const CkMemAsk& ask) {
    CkMemAdmit r = {ask.extra_bytes, st.free_bytes, false};
    if (ask.rhs_bytes > st.rhs_bytes) {
        if (st.arena) {
            r.arena_short = ask.rhs_bytes > st.arena_size - st.arena_used;
        } else {
            r.need += ask.rhs_bytes;
            r.avail += st.rhs_bytes;   // released before the larger one is taken
        }
    }
    if (ask.schur_order > 0 && ask.schur_order != st.schur_order) {
        r.need += ck_host_schur_bytes(ask.schur_order);
        r.avail += ck_host_schur_bytes(st.schur_order);   // schur_ensure releases these first
    }
    if (ask.slab_bytes > st.slab_bytes) {
        r.need += ask.slab_bytes;
        r.avail += st.slab_bytes;
    }
    return r;
}

// ---------------------------------------------------------------------------------------
// leave-group-out cross-validation: members, gather list, tile map and system offsets of the folds
// ---------------------------------------------------------------------------------------
int ck_host_fold_plan(int i, int n_procs, const int64_t n[2], int64_t n0p, const int64_t* perm0, const int64_t* perm1,
                      const int32_t* fold0, const int32_t* fold1, int32_t n_folds, int fold_max, CkFoldPlan* out) {
    if (!out) return ck_fail("ck_cv_folds: null plan");
    if (n_procs < 1 || n_procs > 2 || i < 0 || i >= n_procs) return ck_fail("ck_cv_folds: process index out of range");
    if (n_folds < 1) return ck_fail("ck_cv_folds: n_folds = " + std::to_string(n_folds) + "; at least one fold is needed");
    const int32_t* fold[2] = {fold0, n_procs == 2 ? fold1 : nullptr};
    const int64_t* perm[2] = {perm0, perm1};
    if (!fold[i]) return ck_fail("ck_cv_folds: the fold labels of the predicted process " + std::to_string(i) + " are null");
    *out = CkFoldPlan();
    std::vector<int32_t> cnt((size_t)n_folds, 0), cnt_i((size_t)n_folds, 0);
    for (int k = 0; k < n_procs; ++k) {
        if (!fold[k]) continue;
        for (int64_t a = 0; a < n[k]; ++a) {
            const int32_t f = fold[k][a];
            if (f < -1 || f >= n_folds)
                return ck_fail("ck_cv_folds: label " + std::to_string(f) + " of datum " + std::to_string(a) + " of process " +
                               std::to_string(k) + " is outside [-1, n_folds = " + std::to_string(n_folds) + ")");
            if (f < 0) continue;
            ++cnt[(size_t)f];
            if (k == i) ++cnt_i[(size_t)f];
        }
    }
    out->off.assign((size_t)n_folds + 1, 0);
    for (int32_t f = 0; f < n_folds; ++f) {
        if (cnt_i[(size_t)f] == 0)
            return ck_fail("ck_cv_folds: fold " + std::to_string(f) + " is empty: it holds no datum of process " + std::to_string(i) +
                           " (and " + std::to_string(cnt[(size_t)f]) + " of the other process)");
        if (cnt[(size_t)f] > fold_max)
            return ck_fail("ck_cv_folds: fold " + std::to_string(f) + " holds " + std::to_string(cnt[(size_t)f]) +
                           " data; a fold may hold at most CK_FOLD_MAX = " + std::to_string(fold_max));
        out->off[(size_t)f + 1] = out->off[(size_t)f] + cnt[(size_t)f];
    }
    const int64_t total = out->off[(size_t)n_folds];
    out->pos.assign((size_t)total, 0);
    out->cidx.assign((size_t)total, -1);
    std::vector<int32_t> fill(out->off.begin(), out->off.end() - 1);
    out->pmin = INT64_MAX;
    for (int k = 0; k < n_procs; ++k) {   // ascending internal position: every fold's members come out sorted
        if (!fold[k]) continue;
        for (int64_t j = 0; j < n[k]; ++j) {
            const int64_t a = perm[k] ? perm[k][j] : j;
            const int32_t f = fold[k][a];
            if (f < 0) continue;
            const int64_t p = (k == 0 ? 0 : n0p) + j;
            const int32_t w = fill[(size_t)f]++;
            out->pos[(size_t)w] = (int32_t)p;
            out->cidx[(size_t)w] = k == i ? (int32_t)a : -1;
            out->pmin = std::min(out->pmin, p);
            out->pmax = std::max(out->pmax, p);
        }
    }
    // ---- gather list: small folds packed into tiles, sorted by their first position
    const int T = CK_HOST_FOLD_TILE;
    out->gbase.assign((size_t)n_folds, 0);
    std::vector<int32_t> sm, bg;
    for (int32_t f = 0; f < n_folds; ++f) (cnt[(size_t)f] <= CK_HOST_FOLD_LDS ? sm : bg).push_back(f);
    std::stable_sort(sm.begin(), sm.end(), [&](int32_t a, int32_t b) { return out->pos[(size_t)out->off[(size_t)a]] < out->pos[(size_t)out->off[(size_t)b]]; });
    std::stable_sort(bg.begin(), bg.end(), [&](int32_t a, int32_t b) { return cnt[(size_t)a] > cnt[(size_t)b]; });
    auto pad_tile = [&]() {
        while (out->gpos.size() % (size_t)T) out->gpos.push_back(out->gpos[out->gpos.size() / T * T]);
    };
    for (int32_t f : sm) {
        const int s = cnt[(size_t)f];
        if ((int)(out->gpos.size() % (size_t)T) + s > T) pad_tile();
        out->gbase[(size_t)f] = (int32_t)out->gpos.size();
        out->small.push_back({(int)out->gpos.size(), s, f, 0});
        for (int q = 0; q < s; ++q) out->gpos.push_back(out->pos[(size_t)(out->off[(size_t)f] + q)]);
    }
    pad_tile();
    out->n_small_tiles = (int64_t)out->gpos.size() / T;
    for (int64_t t = 0; t < out->n_small_tiles; ++t)
        out->tiles.push_back({t * T * T, (int)(t * T), (int)(t * T), T, out->gpos[(size_t)(t * T)]});
    // ---- big folds: their own runs of tiles, written straight into their systems
    long long at = out->n_small_tiles * T * T;
    for (int32_t f : bg) {
        const int s = cnt[(size_t)f];
        const int kq = (int)ck_local_tiled_kq(s, s - 1), ld = (int)ck_local_tiled_ld(kq);   // s + 2 + (s - 1) = 2 s + 1 rows
        const int g0 = (int)out->gpos.size();
        out->gbase[(size_t)f] = g0;
        out->big.push_back({at, s, kq, ld, g0, f, 0});
        for (int q = 0; q < s; ++q) out->gpos.push_back(out->pos[(size_t)(out->off[(size_t)f] + q)]);
        while (out->gpos.size() % (size_t)T) out->gpos.push_back(out->gpos.back());
        const int nt = (s + T - 1) / T;
        for (int tm = 0; tm < nt; ++tm)
            for (int tn = 0; tn <= tm; ++tn)
                out->tiles.push_back({at + (long long)tm * T * ld + (long long)tn * T, g0 + tm * T, g0 + tn * T, ld, out->gpos[(size_t)(g0 + tm * T)]});
        at += ck_local_tiled_matrix(kq);
    }
    out->buffer_doubles = at;
    std::stable_sort(out->tiles.begin(), out->tiles.end(), [](const CkFoldTile& a, const CkFoldTile& b) { return a.pos0 < b.pos0; });
    return 0;
}

// ---- ck_cv_local_folds: the predicted data, their labels, the score groups (ck_host.h) ---------------------------------------
int ck_host_local_cv_plan(const char* name_c, int i, int n_procs, const int64_t n[2], int64_t n0p, const int64_t* perm0,
                          const int64_t* perm1, const int32_t* fold0, const int32_t* fold1, int32_t n_folds, bool buffer_i,
                          CkLocalCvPlan* out) {
    const std::string name = std::string(name_c) + ": ";
    if (!out) return ck_fail(name + "null plan");
    if (n_procs < 1 || n_procs > 2 || i < 0 || i >= n_procs) return ck_fail(name + "process index out of range");
    if (n_folds < 0) return ck_fail(name + "n_folds = " + std::to_string(n_folds) + " is negative");
    const int32_t* fold[2] = {fold0, n_procs == 2 ? fold1 : nullptr};
    const int64_t* perm[2] = {perm0, perm1};
    if (!fold[i] && !buffer_i)
        return ck_fail(name + "the fold labels of the predicted process " + std::to_string(i) + " are null and its buffer is off: every datum "
                       "would predict itself (give labels, or buffer2[" + std::to_string(i) + "] >= 0)");
    *out = CkLocalCvPlan();
    const int64_t n_i = n[i];
    out->size.assign((size_t)n_folds, 0);
    std::vector<int64_t> cnt_i((size_t)n_folds, 0);
    for (int k = 0; k < n_procs; ++k) {
        if (!fold[k]) continue;
        for (int64_t a = 0; a < n[k]; ++a) {
            const int32_t f = fold[k][a];
            if (f < -1 || f >= n_folds)
                return ck_fail(name + "label " + std::to_string(f) + " of datum " + std::to_string(a) + " of process " + std::to_string(k) +
                               " is outside [-1, n_folds = " + std::to_string(n_folds) + ")");
            if (f < 0) continue;
            ++out->size[(size_t)f];
            if (k == i) ++cnt_i[(size_t)f];
        }
    }
    for (int32_t f = 0; f < n_folds; ++f)
        if (cnt_i[(size_t)f] == 0)
            return ck_fail(name + "fold " + std::to_string(f) + " is empty: it holds no datum of process " + std::to_string(i) + " (and " +
                           std::to_string(out->size[(size_t)f]) + " of the other process)");
    // the predicted data in the caller's order, then the groups by a counting sort (stable: ascending inside a group)
    if (fold[i]) {
        out->n_groups = n_folds;
        out->off.assign((size_t)n_folds + 1, 0);
        for (int32_t f = 0; f < n_folds; ++f) out->off[(size_t)f + 1] = out->off[(size_t)f] + cnt_i[(size_t)f];
        out->plist.reserve((size_t)out->off[(size_t)n_folds]);
        for (int64_t a = 0; a < n_i; ++a)
            if (fold[i][a] >= 0) {
                out->plist.push_back((int32_t)a);
                out->fp.push_back(fold[i][a]);
            }
        out->idx.resize(out->plist.size());
        std::vector<long long> fill(out->off.begin(), out->off.end() - 1);
        for (size_t t = 0; t < out->plist.size(); ++t) out->idx[(size_t)fill[(size_t)out->fp[t]]++] = (int32_t)t;
    } else {
        out->n_groups = n_i > 0 ? 1 : 0;
        out->off = {0, (long long)n_i};
        if (n_i == 0) out->off.resize(1);
        out->plist.resize((size_t)n_i);
        out->idx.resize((size_t)n_i);
        for (int64_t a = 0; a < n_i; ++a) out->plist[(size_t)a] = out->idx[(size_t)a] = (int32_t)a;
        out->fp.assign((size_t)n_i, -1);
    }
    const int64_t N = n[0] + (n_procs == 2 ? n[1] : 0);
    out->gself.resize((size_t)N);
    for (int k = 0; k < n_procs; ++k) {
        const int64_t off = k == 0 ? 0 : n0p, soff = k == 0 ? 0 : n[0];
        for (int64_t j = 0; j < n[k]; ++j) out->gself[(size_t)(soff + (perm[k] ? perm[k][j] : j))] = (int32_t)(off + j);
    }
    return 0;
}

// ---- ck_predict_local: size classes, slab offsets and batches (ck_host.h) -----------------------------------------------
void ck_host_local_needs(const int* cnt, int64_t m, int lds_limit, int k_hi, int trend, CkLocalNeeds* out) {
    *out = CkLocalNeeds();
    out->need.assign((size_t)m, 0);
    for (int64_t p = 0; p < m; ++p) {
        const long long k = cnt[p];
        out->k_max = std::max<int64_t>(out->k_max, k);
        if (k == 0) ++out->n_empty;
        long long nd = 0;
        if (k > k_hi) {
            out->tiled.push_back(p);
            nd = ck_local_tiled_doubles(k, trend);
        } else if (k > lds_limit) {
            nd = out->need[(size_t)p] = ((k + 2) * k + (k + 1) / 2 + 2 + 1) & ~1LL;
        }
        out->need_max = std::max(out->need_max, nd);
    }
    std::sort(out->tiled.begin(), out->tiled.end(), [&](int64_t a, int64_t b) { return cnt[a] != cnt[b] ? cnt[a] > cnt[b] : a < b; });
}

void ck_host_local_pair_needs(const int* cnt, int64_t m, int lds_limit, int tile_min, CkLocalNeeds* out) {
    ck_host_local_needs(cnt, m, lds_limit, std::min(tile_min, lds_limit), CK_LOCAL_PAIR_ROWS - 2, out);
}

// elements 0 .. n - 1 in order into batches under the budget: place(e, offset inside its batch); *largest is raised to the
// largest batch sum
template <class Need, class Place>
static void cut_batches(int64_t n, long long budget, Need need, Place place, std::vector<std::pair<int64_t, int64_t>>* batches,
                        long long* largest) {
    int64_t b0 = 0;
    long long acc = 0;
    for (int64_t e = 0; e < n; ++e) {
        if (acc + need(e) > budget && e > b0) {
            batches->push_back({b0, e});
            *largest = std::max(*largest, acc);
            b0 = e;
            acc = 0;
        }
        place(e, acc);
        acc += need(e);
    }
    batches->push_back({b0, n});
    *largest = std::max(*largest, acc);
}

void ck_host_local_plan(const int* cnt, const CkLocalNeeds& nd, long long budget, int trend, CkLocalPlan* out) {
    *out = CkLocalPlan();
    const int64_t m = (int64_t)nd.need.size(), nt = (int64_t)nd.tiled.size();
    out->off.assign((size_t)m, 0);
    cut_batches(
        m, budget, [&](int64_t p) { return nd.need[(size_t)p]; }, [&](int64_t p, long long at) { out->off[(size_t)p] = at; },
        &out->batches, &out->slab_doubles);
    out->sys.resize((size_t)nt);
    if (nt == 0) return;
    cut_batches(
        nt, budget, [&](int64_t t) { return ck_local_tiled_doubles(cnt[nd.tiled[(size_t)t]], trend); },
        [&](int64_t t, long long at) {
            const int k = cnt[nd.tiled[(size_t)t]], kq = (int)ck_local_tiled_kq(k, trend);
            out->sys[(size_t)t] = CkLocalSys{at, k, kq, (int)ck_local_tiled_ld(kq), (int)nd.tiled[(size_t)t]};
        },
        &out->tbatches, &out->slab_doubles);
}

// ---- the dense predictors' host arithmetic (ck_host.h) ----------------------------------------------------------------------
int ck_host_block_members(const int32_t* block, int64_t m, int32_t r, std::vector<int>& off, std::vector<int64_t>& member,
                          int64_t* q_max, int64_t* at) {
    off.assign((size_t)r + 1, 0);
    for (int64_t a = 0; a < m; ++a) {
        if (block[a] < 0 || block[a] >= r) {
            *at = a;
            return CK_HOST_BLOCKS_LABEL;
        }
        ++off[(size_t)block[a] + 1];
    }
    int rc = CK_HOST_BLOCKS_OK;
    *q_max = 0;
    for (int32_t b = 0; b < r; ++b) {
        const int q = off[(size_t)b + 1];
        if (q == 0 && rc == CK_HOST_BLOCKS_OK) {
            *at = b;
            rc = CK_HOST_BLOCKS_EMPTY;
        }
        *q_max = std::max<int64_t>(*q_max, q);
        off[(size_t)b + 1] += off[(size_t)b];
    }
    member.resize((size_t)m);
    std::vector<int> pos(off.begin(), off.end() - 1);
    for (int64_t a = 0; a < m; ++a) member[(size_t)pos[(size_t)block[a]]++] = a;
    return rc;
}

int64_t ck_host_prior_pieces(const int* off, int32_t r, int full, std::vector<long long>& poff) {
    auto n = [&](int64_t b) { return (int64_t)(off[b + 1] - off[b]); };
    auto pieces = [](int64_t pairs) { return (pairs + CK_HOST_PRIOR_PIECE - 1) / CK_HOST_PRIOR_PIECE; };
    poff.assign(1, 0);
    poff.reserve((size_t)(full ? (int64_t)r * (r + 1) / 2 : r) + 1);
    for (int64_t R = 0; R < r; ++R) {
        if (!full) {
            poff.push_back(poff.back() + pieces(n(R) * n(R)));
            continue;
        }
        for (int64_t C = 0; C <= R; ++C) poff.push_back(poff.back() + pieces(n(R) * n(C)));
    }
    return poff.back();
}

int64_t ck_host_block_chunk(int64_t option, int64_t free_bytes, int64_t arena_rest, int64_t held_bytes, int64_t Npad, int64_t m) {
    int64_t chunk = option;
    if (chunk <= 0) {
        const int64_t avail = arena_rest >= 0 ? std::max(arena_rest, held_bytes) : free_bytes / 2 + held_bytes;
        chunk = std::max<int64_t>(avail / (8 * Npad) - CK_HOST_AUX_ALIGN, CK_HOST_AUX_ALIGN);
    }
    return std::min(chunk, m);
}

int64_t ck_host_draw_chunk(int64_t option, int64_t free_bytes, int64_t Mp, int64_t m, bool caller_noise, int64_t n_draws) {
    int64_t chunk = option;
    if (chunk <= 0) {
        chunk = free_bytes / 2 / (8 * (Mp + (caller_noise ? 2 : 1) * m)) / 128 * 128;
        chunk = std::max<int64_t>(128, std::min<int64_t>(chunk, 8192));
    }
    return std::min(chunk, n_draws);
}

int64_t ck_host_coincident_site(const double* pcoords, const int* cmap, const unsigned char* mask, int64_t m) {
    std::vector<std::pair<std::pair<double, double>, int64_t>> key;
    key.reserve((size_t)m);
    for (int64_t j = 0; j < m; ++j)
        if (!mask[j]) key.push_back({{pcoords[2 * cmap[j]], pcoords[2 * cmap[j] + 1]}, j});
    std::sort(key.begin(), key.end());
    int64_t stop = -1;
    for (size_t q = 1; q < key.size(); ++q)
        if (key[q].first.first == key[q - 1].first.first && key[q].first.second == key[q - 1].first.second &&
            (stop < 0 || key[q].second < stop))
            stop = key[q].second;   // the larger internal index of the pair (equal keys are sorted by index)
    return stop;
}

void ck_host_pair_plan(const double* pc0, int64_t m0, const double* pc1, int64_t m1, bool site_order, CkPairPlan* out) {
    *out = CkPairPlan();
    out->m0 = m0;
    out->m1 = m1;
    out->m0p = (m0 + 63) / 64 * 64;
    out->rows = out->m0p + m1;
    out->cmap.assign((size_t)out->rows, -1);
    out->row_of.assign((size_t)(m0 + m1), 0);
    out->xy.assign((size_t)(2 * out->rows), 0.0);
    const double* pc[2] = {pc0, pc1};
    const int64_t mk[2] = {m0, m1}, row0[2] = {0, out->m0p}, stacked0[2] = {0, m0};
    std::vector<int64_t> perm;
    for (int k = 0; k < 2; ++k) {
        out->sorted[k] = site_order && mk[k] >= CK_HOST_PAIR_SORT_MIN;
        if (out->sorted[k]) {
            double lo[2] = {1e300, 1e300}, hi[2] = {-1e300, -1e300};
            ck_host_bounding_box(pc[k], mk[k], lo, hi);
            ck_host_hilbert_order(pc[k], mk[k], lo, hi, perm);
        }
        for (int64_t j = 0; j < mk[k]; ++j) {
            const int64_t c = out->sorted[k] ? perm[(size_t)j] : j, r = row0[k] + j;
            out->cmap[(size_t)r] = (int)(stacked0[k] + c);
            out->row_of[(size_t)(stacked0[k] + c)] = r;
            out->xy[(size_t)(2 * r)] = pc[k][2 * c];
            out->xy[(size_t)(2 * r + 1)] = pc[k][2 * c + 1];
        }
    }
}

int64_t ck_host_pair_coincident(const CkPairPlan& P, const double* pc0, const double* pc1, const unsigned char* mask) {
    // the rows of a process as ck_host_coincident_site wants them: the caller's index within the process per internal position
    const int64_t s0 = ck_host_coincident_site(pc0, P.cmap.data(), mask, P.m0);
    if (s0 >= 0) return s0;
    std::vector<int> own((size_t)P.m1);
    for (int64_t j = 0; j < P.m1; ++j) own[(size_t)j] = P.cmap[(size_t)(P.m0p + j)] - (int)P.m0;
    const int64_t s1 = ck_host_coincident_site(pc1, own.data(), mask + P.m0p, P.m1);
    return s1 >= 0 ? P.m0p + s1 : -1;
}

void ck_host_universal_finish(const double* W, const double* beta, const double* Ainv, const double* f0, const int64_t* pperm,
                              double c0, int64_t m, int p, int pi, int offi, double* pred, double* pred_err) {
    ck_host_parallel(m, [&](int, int64_t a, int64_t e) {
        double r[CK_HOST_TREND_QMAX];
        for (int64_t s = a; s < e; ++s) {
            const int64_t c = pperm ? pperm[s] : s;
            const double* wr = &W[s * (p + 2)];
            for (int j = 0; j < p; ++j) r[j] = -wr[2 + j];
            for (int j = 0; j < pi; ++j) r[offi + j] += f0[c * pi + j];
            double pr = wr[1], var = c0 - wr[0];
            for (int j = 0; j < p; ++j) {
                pr += r[j] * beta[j];
                double t = 0.0;
                for (int l = 0; l < p; ++l) t += Ainv[j * p + l] * r[l];
                var += r[j] * t;
            }
            pred[c] = pr;
            pred_err[c] = ck_host_err_of(var);
        }
    });
}

// ---- ck_predict_local_blocks: the member layout (ck_host.h) ----------------------------------------------------------------
int ck_host_local_block_layout(const double* centres, int32_t r, const double* pcoords, int64_t m, const int32_t* block,
                               const double* weight, int pad, CkLocalBlockLayout* out) {
    *out = CkLocalBlockLayout();
    const std::string name = "ck_predict_local_blocks: ";
    if (r < 1) return ck_fail(name + "r must be >= 1, got " + std::to_string(r));
    if (m < 1 || m > INT32_MAX) return ck_fail(name + "m must be in [1, 2^31), got " + std::to_string(m));
    if (pad < 1) pad = 1;
    for (int64_t e = 0; e < 2 * (int64_t)r; ++e)
        if (!std::isfinite(centres[e]))
            return ck_fail(name + "coordinate " + std::to_string(e % 2) + " of centre " + std::to_string(e / 2) + " is not finite (" +
                           std::to_string(centres[e]) + ")");
    int64_t at = 0;
    const int fault = ck_host_block_members(block, m, r, out->off, out->perm, &out->q_max, &at);
    // the first site at fault is reported, its label before its weight and coordinates
    for (int64_t a = 0; a < (fault == CK_HOST_BLOCKS_LABEL ? at : m); ++a) {
        if (!std::isfinite(weight[a]))
            return ck_fail(name + "weight of site " + std::to_string(a) + " is not finite (" + std::to_string(weight[a]) + ")");
        for (int c = 0; c < 2; ++c)
            if (!std::isfinite(pcoords[2 * a + c]))
                return ck_fail(name + "coordinate " + std::to_string(c) + " of site " + std::to_string(a) + " is not finite (" +
                               std::to_string(pcoords[2 * a + c]) + ")");
    }
    if (fault == CK_HOST_BLOCKS_LABEL)
        return ck_fail(name + "block label " + std::to_string(block[at]) + " of site " + std::to_string(at) + " is outside [0, " +
                       std::to_string(r) + ")");
    if (fault == CK_HOST_BLOCKS_EMPTY) return ck_fail(name + "block " + std::to_string(at) + " has no site");
    out->mpad = (m + pad - 1) / pad * pad;
    out->xy.assign((size_t)(2 * out->mpad), 0.0);
    out->w.assign((size_t)out->mpad, 0.0);
    for (int64_t k = 0; k < m; ++k) {
        const int64_t a = out->perm[(size_t)k];
        out->xy[2 * (size_t)k] = pcoords[2 * a];
        out->xy[2 * (size_t)k + 1] = pcoords[2 * a + 1];
        out->w[(size_t)k] = weight[a];
    }
    return 0;
}

// ---- the Vecchia likelihood: ranks -> positions, of the data and of the sites (ck_host.h) ---------------------------------
// ranks (distinct integers) -> positions 0 .. N - 1; two equal ranks: -1 and both data in dup
static int vecchia_positions(const int64_t* rank, int64_t N, std::vector<int>& pos, int64_t dup[2]) {
    pos.resize((size_t)N);
    std::vector<char> seen((size_t)N, 0);
    bool direct = true;
    for (int64_t t = 0; t < N && direct; ++t) {
        const int64_t r = rank[t];
        if (r < 0 || r >= N || seen[(size_t)r]) {
            direct = false;
        } else {
            seen[(size_t)r] = 1;
            pos[(size_t)t] = (int)r;
        }
    }
    if (direct) return 0;
    std::vector<int64_t> ix((size_t)N);
    for (int64_t t = 0; t < N; ++t) ix[(size_t)t] = t;
    std::sort(ix.begin(), ix.end(), [&](int64_t a, int64_t b) { return rank[a] != rank[b] ? rank[a] < rank[b] : a < b; });
    for (int64_t j = 0; j < N; ++j) {
        if (j > 0 && rank[ix[(size_t)j]] == rank[ix[(size_t)(j - 1)]]) {
            dup[0] = ix[(size_t)(j - 1)];
            dup[1] = ix[(size_t)j];
            return -1;
        }
        pos[(size_t)ix[(size_t)j]] = (int)j;
    }
    return 0;
}

int ck_host_vecchia_order(const int64_t* rank, int n_procs, const int64_t n[2], int64_t n0p, int64_t npad, const int64_t* perm0,
                          const int64_t* perm1, CkVecchiaOrder* out) {
    *out = CkVecchiaOrder();
    const int64_t N = n[0] + (n_procs == 2 ? n[1] : 0);
    if (vecchia_positions(rank, N, out->pos, out->dup)) return -1;
    out->rs.assign((size_t)npad, INT32_MAX);
    out->gself.resize((size_t)N);
    for (int k = 0; k < n_procs; ++k) {
        const int64_t off = k == 0 ? 0 : n0p, soff = k == 0 ? 0 : n[0];
        const int64_t* perm = k == 0 ? perm0 : perm1;
        for (int64_t j = 0; j < n[k]; ++j) {
            out->rs[(size_t)(off + j)] = out->pos[(size_t)(soff + perm[j])];
            out->gself[(size_t)(soff + perm[j])] = (int)(off + j);
        }
    }
    return 0;
}

// ---- conditional simulation in the moving neighbourhood: the stacked sites on the augmented set (ck_host.h) ---------------
int ck_host_sim_order(const int64_t* rank, const int64_t m[2], CkSimSites* out) {
    *out = CkSimSites();
    const int64_t mt = m[0] + m[1];
    std::vector<int64_t> ident((size_t)std::max(m[0], m[1]));
    for (size_t t = 0; t < ident.size(); ++t) ident[t] = (int64_t)t;
    CkVecchiaOrder ord;   // the sites as the "data" of an ordering: process 0's, then process 1's
    if (ck_host_vecchia_order(rank, 2, m, m[0], mt, ident.data(), ident.data(), &ord)) {
        out->dup[0] = ord.dup[0];
        out->dup[1] = ord.dup[1];
        return -1;
    }
    out->pos = std::move(ord.pos);
    return 0;
}

void ck_host_sim_ext(int n_procs, const int64_t n[2], const int64_t m[2], int64_t n0p, int64_t npad, const int64_t* perm0,
                     const int64_t* perm1, CkSimSites* out) {
    const int64_t N = n[0] + (n_procs == 2 ? n[1] : 0), mt = m[0] + m[1];
    out->ext.assign((size_t)npad, -1);
    out->rs.assign((size_t)npad, INT32_MAX);
    out->rp.resize((size_t)mt);
    for (int k = 0; k < n_procs; ++k) {
        const int64_t off = k == 0 ? 0 : n0p, soff = k == 0 ? 0 : n[0], moff = k == 0 ? 0 : m[0];
        const int64_t* perm = k == 0 ? perm0 : perm1;
        for (int64_t j = 0; j < n[k] + m[k]; ++j) {
            const int64_t e = perm[j];
            if (e >= n[k]) {
                const int64_t s = moff + (e - n[k]);
                out->ext[(size_t)(off + j)] = (int)(N + s);
                out->rs[(size_t)(off + j)] = (int)(N + out->pos[(size_t)s]);
            } else {
                out->ext[(size_t)(off + j)] = out->rs[(size_t)(off + j)] = (int)(soff + e);
            }
        }
    }
    for (int64_t t = 0; t < mt; ++t) out->rp[(size_t)t] = (int)(N + out->pos[(size_t)t]);
}

// ---- conditional simulation in the moving neighbourhood: the levels of the recursion -------------------------------------
int64_t ck_host_sim_levels(int64_t m, int ld, const int32_t* pos, const int32_t* ns, const int32_t* nbr, CkSimLevels* out) {
    *out = CkSimLevels();
    std::vector<int32_t> at((size_t)m, -1);   // the caller's index of the site at every position
    for (int64_t t = 0; t < m; ++t) {
        if (pos[t] < 0 || pos[t] >= m || at[(size_t)pos[t]] != -1) {
            out->off = {t, (int64_t)pos[t]};
            return -1;
        }
        at[(size_t)pos[t]] = (int32_t)t;
    }
    out->level.assign((size_t)m, 0);
    std::vector<int32_t> lev_at((size_t)m, 0);   // by position
    int32_t n_levels = 0;
    for (int64_t q = 0; q < m; ++q) {
        const int64_t t = at[(size_t)q];
        int32_t lv = 0;
        if (ns[t] < 0 || ns[t] > ld) {
            out->off = {t, (int64_t)ns[t]};
            return -1;
        }
        for (int32_t j = 0; j < ns[t]; ++j) {
            const int32_t u = nbr[t * ld + j];
            if (u < 0 || u >= q) {
                out->off = {t, (int64_t)u};
                return -1;
            }
            lv = std::max(lv, lev_at[(size_t)u]);
        }
        lev_at[(size_t)q] = out->level[(size_t)t] = lv + 1;
        n_levels = std::max(n_levels, lv + 1);
    }
    // counting sort by level; the positions are walked upwards, so a level's sites come out in ascending position
    out->off.assign((size_t)n_levels + 1, 0);
    for (int64_t t = 0; t < m; ++t) ++out->off[(size_t)out->level[(size_t)t]];
    for (int32_t l = 1; l <= n_levels; ++l) out->off[(size_t)l] += out->off[(size_t)(l - 1)];
    out->order.resize((size_t)m);
    std::vector<int64_t> fill(out->off.begin(), out->off.end() - 1);
    for (int64_t q = 0; q < m; ++q) {
        const int32_t t = at[(size_t)q];
        out->order[(size_t)fill[(size_t)(out->level[(size_t)t] - 1)]++] = t;
    }
    return n_levels;
}
