// ck_api.hip -- the C ABI of libcokrige_hip.so (include/cokrige.h): handle, device storage,
// and the host-side drivers of the blocked algorithms.
//
// Storage (all FP64, row-major):
//   Sigma / L   lower block triangle in packed block columns ("panels") of width NB = 512:
//               panel K holds rows [K*NB, Npad) x cols [K*NB, (K+1)*NB), ld = NB.  With
//               world > 1 a process owns the panels K % world == rank.  Npad = N rounded up
//               to NB; padded rows/cols carry an identity so no kernel needs edge code.
//   aux         the right-hand-side rows c0^T (one row per prediction site) and z^T, in the
//               same panel format: aux panel K is mpad x NB at aux + K*mpad*NB.
// Algorithm: right-looking blocked Cholesky on the tall matrix [Sigma; c0^T; z^T]
// (the forward substitution of cho_solve IS the panel step applied to the extra rows),
// two-level blocking NB = 512 / IB = 64, trailing updates on FP64 MFMA.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <atomic>
#include <memory>
#include <string>
#include <utility>
#include <thread>
#include <vector>

#include "../../include/cokrige.h"
#include "ck_devbuf.h"
#include "ck_host.h"
#include "ck_internal.h"
#include "ck_tilemap.h"
#include "ck_model.h"
#include "ck_vecchia.h"

static int64_t roundup(int64_t x, int64_t a) { return (x + a - 1) / a * a; }
#define CK_N_TIMINGS 144
// ck_host_gls's relative pivot threshold: a trend column whose pivot is not above 1e-10 of its diagonal is refused
#define CK_TREND_TOL 1e-10
static_assert(CK_LU_PMAX == 2 * CK_TREND_PMAX, "the local kernels size their LDS by CK_LU_PMAX trend columns");

static int fail(const std::string& msg) { return ck_fail(msg); }   // thread-local text: ck_host.cpp (ck_last_error)
#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(std::string(#expr) + ": " + hipGetErrorString(e_) + " (" __FILE__ ":" +   \
                        std::to_string(__LINE__) + ")");                                          \
    } while (0)
#define CHKH(h)                       \
    if (!(h)) return fail("null handle"); \
    HIPCHK(hipSetDevice((h)->device))

// milliseconds between two recorded events: the form for HIPCHK, and the form of the sites that ignore the status
static hipError_t elapsed_ms(hipEvent_t a, hipEvent_t b, double* out) {
    float ms = 0;
    const hipError_t e = hipEventElapsedTime(&ms, a, b);
    *out = ms;
    return e;
}
static double elapsed_ms(hipEvent_t a, hipEvent_t b) {
    double ms = 0;
    (void)elapsed_ms(a, b, &ms);
    return ms;
}
static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

struct EvPair {
    hipEvent_t a, b;
};

// What the last call left in the right-hand sides (ck_handle::aux_state).  Only AUX_PREDICT feeds ck_verify_model; the states
// with a name in aux_state_text are refused by ck_aux_finish and ck_verify_model until the next ck_predict / ck_aux_begin.
enum AuxState {
    AUX_NONE,        // nothing usable
    AUX_ASSEMBLED,   // right-hand sides assembled (ck_aux_begin), not solved
    AUX_PREDICT,     // solved by ck_predict: rows = V^T, row m = y
    AUX_BLOCKS,      // block sums (or a chunk's unsolved point rows after a failure): the sites are gone
    AUX_LOGLIK,      // y, the trend rows (REML) and the unit rows of every internal position
    AUX_UNIVERSAL,   // ck_predict's rows with the trend rows behind the data row
    AUX_FOLDS,       // y and the unit rows of the withheld positions
    AUX_PAIR,        // ck_predict_pair's stacked rows of both processes, row m0p + m1 = y
    AUX_N_STATES
};
// per state: the entry point that left it (null: none to name) and the clause ck_verify_model adds to the name
static const struct {
    const char *call, *clause;
} aux_state_text[AUX_N_STATES] = {
    {nullptr, nullptr},
    {nullptr, nullptr},
    {nullptr, nullptr},
    {"ck_predict_blocks", "whose right-hand sides are block sums"},
    {"ck_loglik", "whose right-hand sides are the data sites' unit rows"},
    {"ck_predict_universal", "for which the simple-kriging verdict does not apply"},
    {"ck_cv_folds", "whose right-hand sides are the withheld data's unit rows"},
    {"ck_predict_pair", "whose right-hand sides are the stacked sites of both processes"},
};

struct ck_handle {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // arena
    char* arena = nullptr;
    int64_t arena_size = 0, arena_used = 0;
    // model
    int n_procs = 0;
    int metric = CK_METRIC_HAVERSINE;
    CkMatern blk[3];
    DevBuf<CkMatern> d_blk;
    bool model_set = false;
    // partition
    int rank = 0, world = 1;
    // data
    std::vector<double> h_coords[2], h_values[2];
    int64_t n[2] = {0, 0};
    bool data_set[2] = {false, false};
    int64_t N = 0, Npad = 0;      // N: observations; Npad: padded order of the internal matrix
    int64_t n0p = 0, nend = 0;    // internal order: process 0 in [0, n0), process 1 in [n0p, nend)
    int nK = 0;
    bool layout_ready = false;
    // option "site_order": 1 = the sites of each process (and large sets of prediction points) are
    // laid out along a Hilbert curve, so that the 64 rows / columns of an assembly tile are
    // neighbours in space and the lanes of a wave look up neighbouring table intervals; 0 = the
    // caller's order.  perm[k][j] = caller's index of the site at internal position j of process k.
    int site_order = 1;
    std::vector<int64_t> perm[2], pperm;
    bool p_sorted = false;
    DevBuf<double> s0, z;               // stacked sites (3 x Npad) / values (Npad)
    double *s1 = nullptr, *s2 = nullptr;   // rows 1 and 2 of s0
    DevBuf<double> su;                  // chord vectors of the stacked sites (3 x Npad)
    DevBuf<double> pu;                  // chord vectors of the prediction sites (3 x mpad)
    // tabulated correlation (fast assembly)
    CkTable tab[3];
    DevBuf<double> d_coef[3];
    DevBuf<CkTable> d_tabs;
    DevBuf<double*> d_coefptr;
    bool tables_built = false;
    bool tables_stale = false;   // ck_set_model changed the model after the tables were built: rebuild before the next use
    double qbox = 0.0;           // squared bounding-box diagonal of the data sites (Euclidean table range)
    bool exact_cov = false;             // option "exact_cov": bypass the tables
    CkWorklist wl = {nullptr, nullptr, 0, nullptr};   // entries deferred by the table kernels
    DevBuf<int2> wl_items;                   // its list
    DevBuf<unsigned> wl_counts;              // its two counters (used alternately: next_worklist)
    int64_t fallback_total = 0;
    // sig, d_sigptr, d_panelptr, d_info, aux are views (SchurSwap / AuxSwap re-point them); what they look at is owned by
    // sig_slab, sigptr_own, panelptr_own, d_coop, aux_own
    std::vector<double*> sig;    // per panel; nullptr if not owned
    DevBuf<char> sig_slab;       // the owned panels, one allocation
    double** d_sigptr = nullptr;
    double** d_panelptr = nullptr;   // where panel K can be read on this rank: own storage or receive buffer K & 1
    DevBuf<double*> sigptr_own, panelptr_own;
    DevBuf<int> d_tile0, d_panel_of;   // assembly launch map of the owned panels
    DevBuf<int> d_strip_order;         // the same strips sorted by Matern block (work-queue form of the assembly)
    int n_owned = 0, total_tiles = 0;
    // receive slots for remote panels (world > 1): panel K lands in slot K % recv_slots.  Two slots carry the per-panel
    // look-ahead schedule; 2 G slots the grouped one (the G panels of the group being applied + the G being received)
    int recv_slots = 2;
    std::vector<DevBuf<double>> recv;
    long long* d_info = nullptr;
    bool assembled = false, factored = false;
    // aux
    int i_pred = 0;
    int64_t m = 0, mpad = 0;
    double* aux = nullptr;
    DevBuf<double> aux_own;
    DevBuf<double> p0, d_pred, d_pcoords;   // p0: 3 x mpad, d_pred: pred | err, d_pcoords: 2 x mpad
    double *p1 = nullptr, *p2 = nullptr, *d_err = nullptr;
    int64_t p_cap = 0;        // the mpad that p0, pu, d_pcoords and d_pred hold
    DevBuf<char[24]> mv_buf;   // ck_model_variogram's device arrays (lag | out | i | j, 24 bytes per row), kept between the cost
                               // evaluations of a fit
    AuxState aux_state = AUX_NONE;
    double par_sigma[2] = {0.0, 0.0}, par_rho = 0.0;   // ck_set_model's sigma and rho12 (ck_loglik's derivatives in them)
    DevBuf<CkMatern> d_lik_blk;                         // lik_blocks: 3 blocks x (the block, nu - 2 d, nu - d, nu + d, nu + 2 d)
    CkMatern lik_hb[15];                                // ... and what its upload reads
    // ck_predict_blocks: the block rows (the aux panel layout with bmpad = roundup(r + 1, CK_AUX_ALIGN) rows per panel), kept
    // between calls like aux; option "block_chunk": prediction sites per K2 assembly (0: from the device memory the handle may use)
    DevBuf<double> baux;
    int64_t block_chunk = 0;
    int64_t sim_free_bytes = 0;   // option "sim_free_bytes" (tests): the device memory ck_simulate_local counts as free (0: what is free)
    int64_t draw_chunk = 0;   // option "draw_chunk": draws per product launch of ck_conditional_draws (0: from the free device memory)
    // Schur complement of the prediction sites (ck_verify_model), kept between calls with the same padded order
    struct Schur {
        int64_t M = 0;
        int tiles = 0;
        std::vector<DevBuf<double>> panels;
        std::vector<double*> sig;   // the panels as SchurSwap hands them to the sweeps
        DevBuf<double*> d_ptr, d_coefptr;
        DevBuf<int> d_tile0, d_panel_of;
        DevBuf<double> pc, c, u;
        DevBuf<CkMatern> d_blk;
        DevBuf<CkTable> d_tabs;
        DevBuf<long long> d_info;
    } sch;
    // empirical variogram state (ck_vario_*)
    std::vector<double> vg_ci, vg_cj, vg_vi, vg_vj;   // host copies of coordinates / residuals in the device's point order
                                                      // (the pairs the kernels leave to the host are decided on these)
    struct Vario {   // the device side, ck_vario_begin .. ck_vario_end
        DevBuf<double> iu, iv, ju_own, jv_own;
        double *ju = nullptr, *jv = nullptr;   // field j: ju_own / jv_own, or iu / iv when vg_same
        DevBuf<unsigned long long> best;       // extreme-pair hints of the extent pass (ck_vario.hip)
        DevBuf<double> jb, ib64, jbsub;        // bounding balls: 1024-point "j" chunks, 64-point "i" blocks (wave tiles),
                                               // 128-point sub-chunks
        DevBuf<CkVarioExt> part;
        DevBuf<double> psum;
        DevBuf<unsigned long long> pcnt;
        DevBuf<double> out;          // xa[38] | xb[38] | dthr[38] | sums[36] | counts[37] (8-byte words) | kernel arguments
        DevBuf<CkVarioPair> list;    // pairs left to the host; its capacity is what the kernels may fill
        DevBuf<unsigned> count;
    } vg;
    int64_t vg_ni = 0, vg_nj = 0;
    int vg_same = 0, vg_bgrid = 0;
    int64_t vg_stats[4] = {0, 0, 0, 0};   // host-decided pairs of the extent pass | of the binning pass | pairs visited by
                                          // the binning pass | extra extent rounds
    // timings
    double t_ms[CK_N_TIMINGS] = {};   // ck_timings; [16 ..] ck_predict_blocks, [24 ..] ck_loglik, [30 ..] ck_conditional_draws
    int time_gemm = 0;   // 1: bracket every trailing-update launch with events | 2: the Sigma updates only (step-wise form)
    std::vector<EvPair> gemm_ev;
    size_t gemm_ev_used = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
    // look-ahead: the panel step of column K+1 runs on a second (high-priority) stream under the
    // trailing update of panel K
    hipStream_t side = nullptr;
    hipStream_t side_lo = nullptr;    // a second stream of ordinary priority (option "fused_prio" = 2)
    int fused_sweeps_opt = -1;        // ck_factor_predict: -1 automatic (overlapped up to 128 panels) | 0 sequential | 1 overlapped
    int fused_prio = 0;               // ck_factor_predict: which sweep runs on the high-priority stream (fused_sweeps)
    int fused_group = 0;              // ck_factor_predict: panels per group, 0 = as ck_factor
    int group_first = -1, group_tail = 0, group_tail_panels = 0;   // group_plan(): first group (-1 automatic) / last panels with other group sizes
    int assemble_queue = -1;          // option "assemble_queue": resident workgroups of the table-path assembly kernels on a work queue
                                      // (-1 automatic: 768 from 8 strips per workgroup on; 0 = one strip per workgroup)
    int tall_sweep = 1;               // ck_factor_predict: ONE sweep over the tall matrix [Sigma; c0^T; z^T] (tall_sweeps, round 4)
    int tall_split = 2;               // tall sweep, panel steps hidden under a bulk update: cooperative launch on the 512 x 512 head only,
                                      // every other row (Sigma's and the right-hand sides') through k_panel_rows_all (0: never, 1: every
                                      // panel, 2: panels behind the first group with at least tall_split_rows rows)
    int tall_split_rows = 24 * CK_NB; // tall_split 2: shorter panels keep the one cooperative launch
    int solve_la = -1;                // ck_predict's sweep with the chain of the next group under the bulk of the current one (-1: from 40 panels)
    int tall_b2_stream = 1;           // tall sweep: B2(g) on the handle's own stream beside B1(g)
    std::vector<hipEvent_t> ev_b2;
    int tall_thin = 1;                // tall sweep: a last right-hand-side tile row with <= 16 rows in front of the padding computes those only
    int fused_la = -1;                // ck_factor_predict: look-ahead inside the factorisation (fused_sweeps_la); -1: from 40 panels
                                      // (N = 40 000: 522.3 -> 518.1 ms, three interleaved repetitions; N = 10 000: no difference)
    std::vector<hipEvent_t> ev_col, ev_pan;   // [K]: column K fully updated | panel K done
    // option "panel_group": G panels are factored (left-looking inside the group) before the trailing
    // matrix is updated ONCE with K = 512 G (ck_la.hip: gemm_tile_m); 1 = update after every panel
    int panel_group = 0;   // 0 = automatic (eff_group): 4 from 40 panels, 2 from 14, else 1 (measured: the one-column
                           // in-group launches cost more than the saved C traffic on small matrices)
    int64_t local_slab_mb = 0;   // option "local_slab_mb": scratch budget of ck_predict_local (0 = automatic)
    int local_tile_min = 64;     // option "local_tile_min": neighbourhoods larger than this take the tiled path
    int64_t local_nmax[2] = {0, 0};   // ck_set_local_neighbours: nearest-neighbour cap per process of the local predictor (0: none)
    int local_select_cap = 0;    // option "local_select_cap": candidates per process the select pass keeps in LDS (0: the compiled capacity)
    int local_group = 4;         // option "local_group": 64-column blocks per trailing update of the tiled path
    int local_left = 1;          // option "local_left": the tiled path's groups are updated left-looking (one pass with K = g0 in front
                                 // of each group) instead of right-looking (a K = 64 G update of everything behind each group)
    int panel_fused = 2 | 16;         // option "panel_fused", bit 0: factorisation, bit 1: right-hand-side rows --
                                      // left-looking 64-column sub-blocks inside a panel, fused launches (measured at
                                      // N = 40 000: solve sweep 228.2 -> 219.6 ms, factorisation 362.9 -> 365.0 ms);
                                      // bit 4: the whole panel step of the factorisation in one launch of cooperating
                                      // workgroups (k_panel_coop: 360.4 -> 350.0 ms; N = 10 000: 14.4 -> 12.8 ms)
    int64_t loo_g0 = -1;              // >= 0 during ck_loocv: right-hand-side row 1 + p is the unit vector of site loo_g0 + p
    DevBuf<double> d_chunkb;          // chunk bounds of the sites for the radius search (ck_local.hip: lp_chunk_far)
    DevBuf<double> local_slab;        // scratch of ck_predict_local, kept between calls (allocating tens of GiB
                                      // costs up to seconds, erratically); grows when a call needs more
    // option "lookahead": the panel step of column K + 1 on a second stream under the trailing update of the columns beyond
    // it (per-panel updates, no grouping).  With 24 launches per panel step it gained nothing (the side queue's launches
    // starve behind the resident update kernel); with the ONE-launch cooperative panel step, submitted in front of
    // the update, it does where the update is short against the panel step: factor_ms at N = 10 000: 12.8 -> 11.4,
    // N = 18 000: 44.9 -> 41.6, N = 28 000: 130.7 -> 127.9, N = 40 000: 351.5 (groups of 3) against 356.8.
    // -1 = automatic: on for the factorisation from 12 to 63 panels when the panel step is cooperative and no panel_group is
    // forced; 0 / 1 = off / on (1 also switches the solve sweep's variant on)
    int lookahead = -1;
    // the cooperative panel step (ck_la.hip: k_panel_coop, option "panel_fused" bit 4): [0..15] its flags, [16] its error word
    DevBuf<unsigned> d_coop;
    DevBuf<unsigned long long> d_stamps;      // option "gemm_stamps": lifetime stamps of the trailing-update workgroups
    size_t n_stamps = 0;                      // (ck_debug_gemm_clock), 4 words per workgroup of the largest launch
    int64_t stamp_grid[4] = {0, 0, 0, 0};     // grid x, y, J0, panels of the last stamped launch
    int stamp_sel = 0;                        // 1: every launch | >= 2: only the trailing launch behind panel group K0 = stamp_sel - 2
    unsigned coop_seq = 0;
    unsigned coop_spins = 2000000;    // option "coop_spins": polls a workgroup of k_panel_coop spends on one flag before it gives up (~2 s)
    int coop_inject_panel = -1;       // option "coop_inject_panel" (tests): the cooperative step of this panel loses one flag store
    // universal cokriging (ck_set_trend): regressors of process k, n_k x trend_p[k] row-major in the caller's order, kept on the
    // host; d_trendX: their p = sum_k trend_p[k] columns of X as p rows of Npad doubles in the internal order (zero at padding
    // positions and in the other process's rows), uploaded when the layout is known
    std::vector<double> trend_F[2];
    int trend_p[2] = {0, 0};
    bool trend_dirty = false;
    DevBuf<double> d_trendX;
    DevBuf<double> d_univ;          // the universal reduction's output (rows x (q + 1) doubles)
    // measurement-error variances (ck_set_noise): d_a of process k in the caller's order, kept on the host, and the scale s_k;
    // d_noise: [s_k d_a | d_a], two rows of Npad doubles in the internal order (zero at padding positions and where a process
    // has none), uploaded when the layout is known.  noise_on: some s_k d_a > 0 -- otherwise no kernel sees the vector
    std::vector<double> noise_var[2];
    double noise_scale[2] = {1.0, 1.0};
    bool noise_dirty = false, noise_on = false;
    DevBuf<double> d_noise;
    double lik_noise_grad[2] = {0.0, 0.0};   // dl/ds_k of the last ck_loglik / ck_loglik_reml with a gradient
    bool lik_noise_valid = false;            // ... since the last ck_assemble_joint
    int aux_trend = 0;   // trend rows behind the data row of the right-hand sides being assembled (rows m + 1 .. m + aux_trend)
    int loo_dense = 1;   // rows in front of the unit rows in the leave-one-out / likelihood layout (ck_loglik_reml: 1 + p)
    int64_t fisher_product_mb = 0;    // option "fisher_product_mb": room of ck_loglik_fisher's stored products (0: what is free)

    ~ck_handle() {   // events and streams; the buffers release themselves
        for (auto& e : gemm_ev) {
            (void)hipEventDestroy(e.a);
            (void)hipEventDestroy(e.b);
        }
        for (hipEvent_t e : {ev0, ev1, ev2, ev3})
            if (e) (void)hipEventDestroy(e);
        for (const auto* v : {&ev_b2, &ev_col, &ev_pan})
            for (hipEvent_t e : *v) (void)hipEventDestroy(e);
        for (hipStream_t st : {side, side_lo, own_stream})
            if (st) (void)hipStreamDestroy(st);
    }
};
// An entry point that leaves other rows than ck_predict's in the right-hand sides: on every return the layout fields are idle
// again and aux_state names the call.  on_entry: the state also holds while the call runs (it goes through aux_begin_impl more
// than once, or may fail in front of it)
struct CallGuard {
    ck_handle* h;
    AuxState exit_state;
    CallGuard(ck_handle* hh, AuxState st, bool on_entry) : h(hh), exit_state(st) {
        if (on_entry) h->aux_state = st;
    }
    ~CallGuard() {
        h->aux_trend = 0;
        h->loo_g0 = -1;
        h->loo_dense = 1;
        h->aux_state = exit_state;
    }
};
// an admitted call starts its ck_timings slots, and those behind them, from zero
static void timings_from(ck_handle* h, int first) { std::fill(h->t_ms + first, h->t_ms + CK_N_TIMINGS, 0.0); }
static int64_t aux_cap(const ck_handle* h) { return (int64_t)h->aux_own.cap(); }               // doubles
static long long local_slab_doubles(const ck_handle* h) { return (long long)h->local_slab.cap(); }

extern "C" int ck_version(void) { return 103; }
extern "C" int ck_device_count(int* n) {
    HIPCHK(hipGetDeviceCount(n));
    return 0;
}

// ---------------------------------------------------------------------------------------
// memory
// ---------------------------------------------------------------------------------------
static int64_t align256(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }
// What the handle allocates in the caller's arena if there is one (ck_estimate_bytes is the sum of exactly these sizes):
// a panel's rows with the diagonal blocks' inverses behind them (ck_panel_buffer) ...
static_assert(CK_HOST_NB == CK_NB && CK_HOST_PANEL_TAIL == CK_PANEL_TAIL, "ck_host.h and ck_internal.h disagree about a panel");
static_assert(CK_HOST_AUX_ALIGN == CK_AUX_ALIGN && CK_HOST_PRIOR_PIECE == CK_PRIOR_PIECE && CK_HOST_TREND_QMAX == CK_UNIV_QMAX,
              "ck_host.h and ck_internal.h disagree about the dense predictors' constants");
static int64_t panel_payload(int64_t Np, int K) { return ck_host_panel_payload(Np, K); }
static int64_t panel_bytes(int64_t Np, int K) { return align256(panel_payload(Np, K) + CK_PANEL_SLACK_BYTES); }   // in the slab
static int64_t recv_bytes(int64_t Np) { return panel_payload(Np, 0) + CK_PANEL_SLACK_BYTES; }   // a receive slot: any panel
static int64_t site_bytes(int64_t Np) { return 3 * Np * 8; }              // s0, su (p0, pu with mpad)
static int64_t value_bytes(int64_t Np) { return Np * 8; }                 // z
static int64_t ptr_bytes(int nK) { return (int64_t)nK * sizeof(double*); }   // d_sigptr, d_panelptr
static int64_t rhs_bytes(int64_t mpad, int64_t Np) { return mpad * Np * 8; }   // aux
static int64_t pair_bytes(int64_t mpad) { return 2 * mpad * 8; }          // d_pcoords, d_pred
static int64_t schur_bytes(int64_t Mp) { return ck_host_schur_bytes(Mp); }   // what schur_ensure(h, Mp) allocates

// The admission of a call that grows the handle's buffers, in front of its first allocation: what the handle holds and the
// free device memory against the call's right-hand sides, Schur order (0: none), scratch slab and temporaries
// (ck_host_mem_admit has the rule).  The caller words its refusal from the amounts.
static int mem_admit(const ck_handle* h, const CkMemAsk& ask, CkMemAdmit* out) {
    size_t fr = 0, tot = 0;
    HIPCHK(hipMemGetInfo(&fr, &tot));
    const CkMemState st = {(int64_t)fr, h->arena != nullptr, h->arena_size, h->arena_used,
                           aux_cap(h) * 8, h->sch.M, local_slab_doubles(h) * 8};
    *out = ck_host_mem_admit(st, ask);
    return 0;
}

// b <- `bytes` (rounded up to 256) of the arena as a view, or of device memory as its owner; b is empty if that fails.  An
// arena never takes a carve back: a buffer that grows under it abandons the old one
template <class T>
static int dev_alloc(ck_handle* h, DevBuf<T>& b, int64_t bytes) {
    bytes = align256(bytes);
    b.reset();
    if (h->arena) {
        if (h->arena_used + bytes > h->arena_size)
            return fail("arena too small: need " + std::to_string(h->arena_used + bytes) + " bytes, have " +
                        std::to_string(h->arena_size));
        b.view((T*)(h->arena + h->arena_used), (size_t)bytes / sizeof(T));
        h->arena_used += bytes;
        return 0;
    }
    HIPCHK(b.reserve((size_t)bytes / sizeof(T)));
    return 0;
}

extern "C" int ck_create(int device_id, ck_handle** out) {
    if (!out) return fail("null out");
    int nd = 0;
    HIPCHK(hipGetDeviceCount(&nd));
    if (nd <= 0) return fail("no HIP device visible: libcokrige_hip needs an MI355X (gfx950)");
    if (device_id < 0 || device_id >= nd) return fail("bad device id");
    HIPCHK(hipSetDevice(device_id));
    std::unique_ptr<ck_handle> h(new ck_handle());   // the handle cleans up after itself if a step below fails
    h->device = device_id;
    HIPCHK(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    HIPCHK(hipEventCreate(&h->ev0));
    HIPCHK(hipEventCreate(&h->ev1));
    HIPCHK(hipEventCreate(&h->ev2));
    HIPCHK(hipEventCreate(&h->ev3));
    {
        int lo = 0, hi = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIPCHK(hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, hi));
    }
    HIPCHK(h->d_coop.reserve(32));
    HIPCHK(hipMemset(h->d_coop, 0, 32 * sizeof(unsigned)));
    HIPCHK(h->d_blk.reserve(3));
    h->d_info = (long long*)(h->d_coop + 18);   // behind the cooperative step's error word: one 16-byte read-back for both
    *out = h.release();
    return 0;
}

extern "C" int ck_create_partitioned(const int* device_ids, int n_dev, int rank, ck_handle** out) {
    if (!device_ids || n_dev < 1 || rank < 0 || rank >= n_dev) return fail("bad device list / rank");
    if (ck_create(device_ids[rank], out)) return -1;
    (*out)->rank = rank;
    (*out)->world = n_dev;
    return 0;
}

extern "C" int ck_destroy(ck_handle* h) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    if (h->side) (void)hipStreamSynchronize(h->side);
    if (h->side_lo) (void)hipStreamSynchronize(h->side_lo);
    delete h;
    return 0;
}

extern "C" int ck_set_stream(ck_handle* h, void* hip_stream, int external) {
    CHKH(h);
    h->stream = external ? (hipStream_t)hip_stream : h->own_stream;
    return 0;
}

extern "C" int ck_set_arena(ck_handle* h, void* dev_base, int64_t nbytes) {
    CHKH(h);
    // the first allocation an arena could serve is ensure_layout's s0, which is never released (ck_set_data's condition)
    if (h->layout_ready || h->s0) return fail("ck_set_arena must precede any allocation");
    if (((uintptr_t)dev_base & 255) != 0) return fail("arena base must be 256-byte aligned");
    h->arena = (char*)dev_base;
    h->arena_size = nbytes;
    h->arena_used = 0;
    return 0;
}

extern "C" int ck_synchronize(ck_handle* h) {
    CHKH(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// ---------------------------------------------------------------------------------------
// model / data
// ---------------------------------------------------------------------------------------
extern "C" int ck_set_model(ck_handle* h, int n_procs, const double* sigma, const double* nu, const double* len_scale,
                            const double* nugget, double rho12) {
    CHKH(h);
    if (n_procs != 1 && n_procs != 2) return fail("n_procs must be 1 or 2");
    if (!sigma || !nu || !len_scale || !nugget) return fail("null parameter array");
    const int nb = n_procs == 1 ? 1 : 3;
    for (int k = 0; k < nb; ++k)
        if (!(nu[k] > 0.0) || !(len_scale[k] > 0.0)) return fail("nu and len_scale must be positive");
    CkMatern prev[3];
    memcpy(prev, h->blk, sizeof(prev));
    const int prev_procs = h->n_procs;
    ck_model_prepare(n_procs, sigma, nu, len_scale, nugget, rho12, h->blk);
    if (h->tables_built && (prev_procs != n_procs || memcmp(prev, h->blk, sizeof(prev)) != 0)) h->tables_stale = true;
    h->n_procs = n_procs;
    h->par_sigma[0] = sigma[0];
    h->par_sigma[1] = n_procs == 2 ? sigma[1] : 0.0;
    h->par_rho = n_procs == 2 ? rho12 : 0.0;
    HIPCHK(hipMemcpyAsync(h->d_blk, h->blk, 3 * sizeof(CkMatern), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->model_set = true;
    h->assembled = h->factored = false;
    h->aux_state = AUX_NONE;   // solved right-hand sides of the old model must not feed ck_verify_model
    return 0;
}

extern "C" int ck_set_metric(ck_handle* h, int metric) {
    CHKH(h);
    if (metric != CK_METRIC_HAVERSINE && metric != CK_METRIC_EUCLID) return fail("unknown metric");
    if (metric != h->metric) {
        h->metric = metric;
        h->layout_ready = false;   // site transforms depend on the metric
        h->assembled = h->factored = false;
        h->aux_state = AUX_NONE;
    }
    return 0;
}

extern "C" int ck_set_partition(ck_handle* h, int rank, int world) {
    CHKH(h);
    if (world < 1 || rank < 0 || rank >= world) return fail("bad partition");
    if (h->layout_ready) return fail("ck_set_partition must precede ck_assemble_joint");
    h->rank = rank;
    h->world = world;
    return 0;
}

extern "C" int ck_set_data(ck_handle* h, int k, const double* coords, const double* values, int64_t n_k) {
    CHKH(h);
    if (k < 0 || k > 1) return fail("process index must be 0 or 1");
    if (n_k < 0 || (n_k > 0 && (!coords || !values))) return fail("bad data arrays");
    // also after ck_set_metric has invalidated the layout: the site arrays and panels keep their first sizes
    if (h->layout_ready || h->s0) return fail("data already laid out on the device; create a new handle to change it");
    h->h_coords[k].assign(coords, coords + 2 * n_k);
    h->h_values[k].assign(values, values + n_k);
    h->n[k] = n_k;
    h->data_set[k] = true;
    h->trend_F[k].clear();   // new data: the regressors of the old sites no longer apply
    h->trend_p[k] = 0;
    h->noise_var[k].clear();   // ... and neither do their measurement-error variances
    h->noise_scale[k] = 1.0;
    h->noise_dirty = true;
    return 0;
}

extern "C" int ck_set_trend(ck_handle* h, int k, const double* F, int64_t n_k, int p_k) {
    CHKH(h);
    if (k < 0 || k > 1) return fail("ck_set_trend: process index must be 0 or 1");
    if (p_k < 0 || p_k > CK_TREND_PMAX)
        return fail("ck_set_trend: " + std::to_string(p_k) + " regressors for process " + std::to_string(k) + "; at most " +
                    std::to_string(CK_TREND_PMAX) + " per process");
    if (!h->data_set[k]) return fail("ck_set_trend: ck_set_data has not been called for process " + std::to_string(k));
    if (n_k != h->n[k])
        return fail("ck_set_trend: " + std::to_string(n_k) + " rows for process " + std::to_string(k) + ", which has " +
                    std::to_string(h->n[k]) + " data sites");
    if (p_k > 0 && n_k < p_k)
        return fail("ck_set_trend: process " + std::to_string(k) + " has " + std::to_string(n_k) + " data sites for " +
                    std::to_string(p_k) + " regressors");
    if (p_k > 0 && !F) return fail("ck_set_trend: null regressors");
    for (int64_t e = 0; e < n_k * p_k; ++e)
        if (!std::isfinite(F[e]))
            return fail("ck_set_trend: regressor " + std::to_string(e % p_k) + " of process " + std::to_string(k) +
                        " is not finite at data site " + std::to_string(e / p_k));
    if (p_k == 0)
        h->trend_F[k].clear();
    else
        h->trend_F[k].assign(F, F + n_k * p_k);
    h->trend_p[k] = p_k;
    h->trend_dirty = true;
    return 0;
}

extern "C" int ck_set_noise(ck_handle* h, int k, const double* var, int64_t n_k, double scale) {
    CHKH(h);
    if (k < 0 || k > 1) return fail("ck_set_noise: process index must be 0 or 1");
    if (h->world != 1)
        return fail("ck_set_noise is the single-process form: this handle is partitioned (world = " + std::to_string(h->world) +
                    "); process " + std::to_string(k) + " keeps no measurement-error variances");
    if (!h->data_set[k]) return fail("ck_set_noise: ck_set_data has not been called for process " + std::to_string(k));
    const bool clear = !var || n_k == 0;
    if (!clear && n_k != h->n[k])
        return fail("ck_set_noise: " + std::to_string(n_k) + " variances for process " + std::to_string(k) + ", which has " +
                    std::to_string(h->n[k]) + " data sites");
    if (!clear) {
        if (!(std::isfinite(scale) && scale >= 0.0))
            return fail("ck_set_noise: the scale of process " + std::to_string(k) + " is " + std::to_string(scale) +
                        "; it must be finite and >= 0");
        for (int64_t a = 0; a < n_k; ++a)
            if (!(std::isfinite(var[a]) && var[a] >= 0.0))
                return fail("ck_set_noise: the variance of datum " + std::to_string(a) + " of process " + std::to_string(k) + " is " +
                            std::to_string(var[a]) + "; it must be finite and >= 0");
    }
    if (clear) {
        h->noise_var[k].clear();
        h->noise_scale[k] = 1.0;
    } else {
        h->noise_var[k].assign(var, var + n_k);
        h->noise_scale[k] = scale;
    }
    h->noise_dirty = true;
    h->assembled = h->factored = false;   // as ck_set_model: Sigma, its factor and the solved right-hand sides are stale
    h->aux_state = AUX_NONE;
    h->lik_noise_valid = false;
    return 0;
}


// ---------------------------------------------------------------------------------------
// tabulated covariance: build C(q) = amp * rho tables for every Matern block of the model
// (ck_math.h "Tabulated covariance").  Node values come from the exact device evaluator;
// the Chebyshev fit per interval is done here in long double; the result is checked on the
// device against the exact evaluator (k_table_check) and disabled if it misses 2e-13.
// ---------------------------------------------------------------------------------------
static int build_tables(ck_handle* h, double qbox_euclid) {
    const int nblk = h->n_procs == 1 ? 1 : 3;
    if (!h->wl.items) {
        const unsigned cap = 1u << 22;   // 4 M deferred entries (32 MB); beyond that the assembly re-runs exactly
        HIPCHK(h->wl_items.reserve(cap));
        HIPCHK(h->wl_counts.reserve(4));   // two pairs (count, work queue), used alternately: see CkWorklist
        HIPCHK(hipMemset(h->wl_counts, 0, 4 * sizeof(unsigned)));
        h->wl = CkWorklist{h->wl_items, h->wl_counts, cap, h->wl_counts + 2};
    }
    const int ND = CK_TAB_DEG + 1;
    HIPCHK(h->d_tabs.reserve(3));   // allocated by the first call
    HIPCHK(h->d_coefptr.reserve(3));
    for (int b = 0; b < 3; ++b) HIPCHK(h->d_coef[b].reserve((size_t)ND * CK_TAB_STRIDE));
    DevTemps tmp;
    unsigned long long* d_err = nullptr;
    double *d_q = nullptr, *d_f = nullptr;
    HIPCHK(tmp.get(&d_err, (size_t)(8)));
    HIPCHK(tmp.get(&d_q, (size_t)((size_t)ND * CK_TAB_STRIDE * 8)));
    HIPCHK(tmp.get(&d_f, (size_t)((size_t)ND * CK_TAB_STRIDE * 8)));
    std::vector<double> hq(ND * CK_TAB_STRIDE), hf(ND * CK_TAB_STRIDE), hcoef(ND * CK_TAB_STRIDE);
    for (int b = 0; b < 3; ++b) {
        CkTable& T = h->tab[b];
        memset(&T, 0, sizeof(T));
        if (b >= nblk) {
            T = h->tab[0];
            continue;
        }
        const CkMatern& m = h->blk[b];
        int64_t base = 0;
        int n_int = ck_table_plan(&m, h->metric, qbox_euclid, &base, hq.data());
        if (n_int <= 0) continue;
        HIPCHK(hipMemcpyAsync(d_q, hq.data(), (size_t)n_int * ND * 8, hipMemcpyHostToDevice, h->stream));
        ck_launch_table_nodes(h->stream, h->d_blk + b, h->metric, d_q, (int64_t)n_int * ND, d_f);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hf.data(), d_f, (size_t)n_int * ND * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        // node values must be finite (they are: rho underflows to 0 far in the tail)
        bool finite = true;
        for (int64_t i = 0; i < (int64_t)n_int * ND; ++i) finite = finite && (fabs(hf[i]) < 1e300);
        if (!finite) continue;
        ck_table_fit(hf.data(), n_int, base, hcoef.data());
        HIPCHK(hipMemcpyAsync(h->d_coef[b], hcoef.data(), (size_t)ND * CK_TAB_STRIDE * 8, hipMemcpyHostToDevice, h->stream));
        T.base = (int32_t)base;
        T.n_int = n_int;
        T.q_lo = ck_table_edge(base);
        T.q_hi = ck_table_edge(base + n_int);
        HIPCHK(hipMemsetAsync(d_err, 0, 8, h->stream));
        ck_launch_table_check(h->stream, h->d_blk + b, h->metric, T, h->d_coef[b], d_err);
        HIPCHK(hipGetLastError());
        unsigned long long eb = 0;
        HIPCHK(hipMemcpyAsync(&eb, d_err, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        memcpy(&T.max_rel_err, &eb, 8);
        T.enabled = (T.max_rel_err < 2e-13) ? 1 : 0;
    }
    HIPCHK(hipMemcpyAsync(h->d_tabs, h->tab, 3 * sizeof(CkTable), hipMemcpyHostToDevice, h->stream));
    double* const coefs[3] = {h->d_coef[0], h->d_coef[1], h->d_coef[2]};
    HIPCHK(hipMemcpyAsync(h->d_coefptr, coefs, sizeof(coefs), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->tables_built = true;
    return 0;
}

// (thread team, Hilbert order, bounding box, the reference's distance arithmetic, the variogram's level planning and tie
// decisions: ck_host.cpp -- host-only code, also built with the CPU sanitizers by tests/test_host_sanitize.py)
// Decide the padded layout, upload sites / values, allocate the owned panels.
// need_panels = false (ck_predict_local): sites, tables and chunk bounds only -- the local predictor never touches the Sigma
// panels or the receive buffers (a rank pool's local handle used to hold its share of a 40 GB Sigma beside the
// joint runner's arena); they are allocated by the first entry that needs them.
static int ensure_panels(ck_handle* h);
static int ensure_layout(ck_handle* h, bool need_panels = true) {
    if (h->layout_ready) {
        // tables of a model set before the last ck_set_model (a handle kept across models, e.g. the likelihood's)
        if (h->tables_stale && build_tables(h, h->qbox)) return -1;
        h->tables_stale = false;
        return need_panels ? ensure_panels(h) : 0;
    }
    if (!h->model_set) return fail("ck_set_model has not been called");
    for (int k = 0; k < h->n_procs; ++k)
        if (!h->data_set[k]) return fail("ck_set_data missing for process " + std::to_string(k));
    const int64_t n0 = h->n[0], n1 = h->n_procs == 2 ? h->n[1] : 0;
    h->N = n0 + n1;
    if (h->N <= 0) return fail("no observations");
    // process 1 starts on a 64-row tile boundary, so every assembly tile has ONE Matern block
    h->n0p = n1 > 0 ? roundup(n0, 64) : n0;
    h->nend = h->n0p + n1;
    h->Npad = roundup(h->nend, CK_NB);
    h->nK = (int)(h->Npad / CK_NB);
    const int64_t Np = h->Npad;
    if (!h->s0 || !h->su || !h->z) {
        if (dev_alloc(h, h->s0, site_bytes(Np)) || dev_alloc(h, h->su, site_bytes(Np)) || dev_alloc(h, h->z, value_bytes(Np)))
            return -1;
        h->s1 = h->s0 + Np;
        h->s2 = h->s0 + 2 * Np;
    }
    // stage coords -> device, transform
    double blo[2] = {1e300, 1e300}, bhi[2] = {-1e300, -1e300};
    for (int k = 0; k < h->n_procs; ++k) ck_host_bounding_box(h->h_coords[k].data(), h->n[k], blo, bhi);
    std::vector<double> hc(2 * Np, 0.0), hz(Np, 0.0);
    for (int k = 0; k < h->n_procs; ++k) {
        const int64_t nk = h->n[k], off = k == 0 ? 0 : h->n0p;
        if (h->site_order) {
            ck_host_hilbert_order(h->h_coords[k].data(), nk, blo, bhi, h->perm[k]);
        } else {
            h->perm[k].resize((size_t)nk);
            for (int64_t j = 0; j < nk; ++j) h->perm[k][(size_t)j] = j;
        }
        h->trend_dirty = true;   // a new site order (also a re-layout: ck_factor's retry, option "site_order"): X follows it
        h->noise_dirty = true;   // ... and so do the measurement-error variances
        for (int64_t j = 0; j < nk; ++j) {
            const int64_t e = h->perm[k][(size_t)j];
            hc[2 * (off + j)] = h->h_coords[k][2 * e];
            hc[2 * (off + j) + 1] = h->h_coords[k][2 * e + 1];
            hz[off + j] = h->h_values[k][e];
        }
    }
    DevTemps tmp;
    double* d_tmp = nullptr;
    HIPCHK(tmp.get(&d_tmp, (size_t)(2 * Np * 8)));
    HIPCHK(hipMemcpyAsync(d_tmp, hc.data(), 2 * Np * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->z, hz.data(), Np * 8, hipMemcpyHostToDevice, h->stream));
    ck_launch_prep_sites(h->stream, d_tmp, Np, h->metric, h->s0, h->s1, h->s2, h->su);
    HIPCHK(h->d_chunkb.reserve((size_t)(4 * ((h->nend + 255) / 256 + 1))));   // outside the arena: not part of ck_estimate_bytes
    ck_launch_local_chunk_bounds(h->stream, h->su, CkLayout{h->n[0], h->n0p, h->nend, h->Npad}, h->d_chunkb);
    HIPCHK(hipStreamSynchronize(h->stream));
    // squared bounding-box diagonal of the data sites (Euclidean table range)
    const double qbox = (bhi[0] - blo[0]) * (bhi[0] - blo[0]) + (bhi[1] - blo[1]) * (bhi[1] - blo[1]);
    h->qbox = qbox;
    if (build_tables(h, qbox)) return -1;
    h->tables_stale = false;
    h->layout_ready = true;
    return need_panels ? ensure_panels(h) : 0;
}

// Everything is built into locals and handed to the handle at the end: a failed allocation or copy leaves no panel pointers
// behind (sig stays empty, so the next call starts over) and gives the arena back what this call had carved
struct PanelSet {
    std::vector<double*> sig;
    DevBuf<char> slab;
    DevBuf<double*> sigptr, panelptr;
    DevBuf<int> tile0, panel_of, strip_order;
    std::vector<DevBuf<double>> recv;
    int n_owned = 0, total_tiles = 0;
};
static int build_panels(ck_handle* h, PanelSet& s) {
    const int64_t Np = h->Npad;
    s.sig.assign(h->nK, nullptr);
    // the owned panels from ONE allocation (outside a caller's arena, where dev_alloc carves anyway): 79 hipMalloc /
    // hipFree calls of tens of MB each were most of what a cold pass spent in its first assemble and in ck_destroy
    // beyond the kernels (scripts/diag_cold_phases.py)
    int64_t slab_bytes = 0;
    for (int K = h->rank; K < h->nK; K += h->world) slab_bytes += panel_bytes(Np, K);
    if (dev_alloc(h, s.slab, slab_bytes)) return -1;
    char* slab = s.slab;
    for (int K = h->rank; K < h->nK; K += h->world) {
        s.sig[K] = (double*)slab;
        slab += panel_bytes(Np, K);
    }
    if (dev_alloc(h, s.sigptr, ptr_bytes(h->nK))) return -1;
    HIPCHK(hipMemcpy(s.sigptr, s.sig.data(), h->nK * sizeof(double*), hipMemcpyHostToDevice));
    std::vector<int> tile0, panel_of;
    int acc = 0;
    for (int K = h->rank; K < h->nK; K += h->world) {
        tile0.push_back(acc);
        panel_of.push_back(K);
        acc += (int)((Np - (int64_t)K * CK_NB) / 64);
    }
    tile0.push_back(acc);
    s.n_owned = (int)panel_of.size();
    s.total_tiles = acc;
    HIPCHK(s.tile0.reserve(tile0.size()));
    HIPCHK(s.panel_of.reserve(panel_of.size() + 1));
    HIPCHK(hipMemcpy(s.tile0, tile0.data(), tile0.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s.panel_of, panel_of.data(), panel_of.size() * sizeof(int), hipMemcpyHostToDevice));
    {
        // work-queue form of the assembly: the 64-row strips of all owned panels sorted by Matern block (block 22 first, then
        // 12, then 11; inside a block back to front as before), so that a resident workgroup reloads its table twice per launch
        std::vector<int> order;
        order.reserve((size_t)acc);
        for (int cls = 2; cls >= 0; --cls)
            for (int j = (int)panel_of.size() - 1; j >= 0; --j) {
                const int64_t K = panel_of[(size_t)j];
                const int pc = K * CK_NB >= h->n0p ? 1 : 0;
                for (int tile = tile0[(size_t)j + 1] - tile0[(size_t)j] - 1; tile >= 0; --tile) {
                    const int64_t rt = K * CK_NB + (int64_t)tile * 64;
                    if ((rt >= h->n0p ? 1 : 0) + pc == cls) order.push_back(tile0[(size_t)j] + tile);
                }
            }
        HIPCHK(s.strip_order.reserve(std::max<size_t>(order.size(), 1)));
        HIPCHK(hipMemcpy(s.strip_order, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    if (h->world > 1) {
        s.recv.resize((size_t)h->recv_slots);
        for (auto& r : s.recv)
            if (dev_alloc(h, r, recv_bytes(Np))) return -1;
    }
    std::vector<double*> pp(h->nK);
    for (int K = 0; K < h->nK; ++K) pp[K] = s.sig[K] ? s.sig[K] : (h->world > 1 ? s.recv[(size_t)(K % h->recv_slots)].get() : nullptr);
    if (dev_alloc(h, s.panelptr, ptr_bytes(h->nK))) return -1;
    HIPCHK(hipMemcpy(s.panelptr, pp.data(), h->nK * sizeof(double*), hipMemcpyHostToDevice));
    return 0;
}
static int ensure_panels(ck_handle* h) {
    if (!h->sig.empty()) return 0;
    const int64_t used0 = h->arena_used;
    PanelSet s;
    if (build_panels(h, s)) {
        h->arena_used = used0;
        return -1;
    }
    h->sig = std::move(s.sig);
    h->sig_slab = std::move(s.slab);
    h->sigptr_own = std::move(s.sigptr);
    h->panelptr_own = std::move(s.panelptr);
    h->d_sigptr = h->sigptr_own;
    h->d_panelptr = h->panelptr_own;
    h->d_tile0 = std::move(s.tile0);
    h->d_panel_of = std::move(s.panel_of);
    h->d_strip_order = std::move(s.strip_order);
    h->recv = std::move(s.recv);
    h->n_owned = s.n_owned;
    h->total_tiles = s.total_tiles;
    return 0;
}

// ---------------------------------------------------------------------------------------
// element-wise parity surface
// ---------------------------------------------------------------------------------------
static int blk_index(ck_handle* h, int i, int j, int* idx) {
    if (!h->model_set) return fail("ck_set_model has not been called");
    if (i < 0 || j < 0 || i >= h->n_procs || j >= h->n_procs) return fail("process index out of range");
    *idx = i + j;
    return 0;
}

static int dense_common(ck_handle* h, int bidx, int add_nugget, int mode, const double* A, int64_t a, const double* B,
                        int64_t b, double* out) {
    if (a <= 0 || b <= 0) return 0;
    DevTemps tmp;
    double *dA = nullptr, *dB = nullptr, *dO = nullptr, *ta = nullptr, *tb = nullptr;
    HIPCHK(tmp.get(&dA, (size_t)(2 * a * 8)));
    HIPCHK(tmp.get(&dB, (size_t)(2 * b * 8)));
    HIPCHK(tmp.get(&ta, (size_t)(3 * a * 8)));
    HIPCHK(tmp.get(&tb, (size_t)(3 * b * 8)));
    HIPCHK(tmp.get(&dO, (size_t)(a * b * 8)));
    HIPCHK(hipMemcpyAsync(dA, A, 2 * a * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(dB, B, 2 * b * 8, hipMemcpyHostToDevice, h->stream));
    ck_launch_prep_sites(h->stream, dA, a, h->metric, ta, ta + a, ta + 2 * a, nullptr);
    ck_launch_prep_sites(h->stream, dB, b, h->metric, tb, tb + b, tb + 2 * b, nullptr);
    ck_launch_cov_dense(h->stream, h->d_blk + bidx, h->metric, add_nugget, mode, ta, ta + a, ta + 2 * a, a, tb, tb + b,
                        tb + 2 * b, b, dO);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dO, a * b * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int ck_distance_dense(ck_handle* h, const double* A, int64_t a, const double* B, int64_t b, double* out) {
    CHKH(h);
    return dense_common(h, 0, 0, 1, A, a, B, b, out);
}

extern "C" int ck_cov_dense(ck_handle* h, int i, int j, const double* A, int64_t a, const double* B, int64_t b,
                            int use_nugget, double* out) {
    CHKH(h);
    int bidx;
    if (blk_index(h, i, j, &bidx)) return -1;
    return dense_common(h, bidx, (i == j) && use_nugget, 0, A, a, B, b, out);
}

extern "C" int ck_cov_lags(ck_handle* h, int i, int j, const double* lags, int64_t n, int use_nugget, double* out) {
    CHKH(h);
    int bidx;
    if (blk_index(h, i, j, &bidx)) return -1;
    if (n <= 0) return 0;
    DevTemps tmp;
    double *dl = nullptr, *dO = nullptr;
    HIPCHK(tmp.get(&dl, (size_t)(n * 8)));
    HIPCHK(tmp.get(&dO, (size_t)(n * 8)));
    HIPCHK(hipMemcpyAsync(dl, lags, n * 8, hipMemcpyHostToDevice, h->stream));
    ck_launch_cov_lags(h->stream, h->d_blk + bidx, (i == j) && use_nugget, dl, n, dO);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dO, n * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int ck_model_variogram(ck_handle* h, const int32_t* pi, const int32_t* pj, const double* lags, int64_t n,
                                  int kind, double* out) {
    CHKH(h);
    if (!h->model_set) return fail("ck_set_model has not been called");
    if (kind != 0 && kind != 1) return fail("kind must be 0 (semivariogram) or 1 (covariogram)");
    if (n <= 0) return 0;
    if (!pi || !pj || !lags || !out) return fail("null array");
    for (int64_t r = 0; r < n; ++r)
        if (pi[r] < 0 || pj[r] < 0 || pi[r] >= h->n_procs || pj[r] >= h->n_procs)
            return fail("process index out of range in row " + std::to_string(r));
    // sill of the cross-semivariogram: nansum(sigma^2 + nugget) / 2 over the parameter arrays (model.py:219-221)
    double sill = h->blk[0].amp + h->blk[0].nugget;
    if (h->n_procs == 2) sill = 0.5 * (sill + (h->blk[2].amp + h->blk[2].nugget));
    else sill = 0.5 * sill;
    // one allocation for all four arrays; a fit calls this hundreds of times with the same n
    if ((size_t)n > h->mv_buf.cap()) HIPCHK(h->mv_buf.reserve((size_t)roundup(n, 256)));
    const size_t mv_cap = h->mv_buf.cap();
    double* dl = reinterpret_cast<double*>(h->mv_buf.get());
    double* dO = dl + mv_cap;
    int* di = reinterpret_cast<int*>(dO + mv_cap);
    int* dj = di + mv_cap;
    HIPCHK(hipMemcpyAsync(di, pi, n * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(dj, pj, n * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(dl, lags, n * 8, hipMemcpyHostToDevice, h->stream));
    ck_launch_model_variogram(h->stream, h->d_blk, sill, kind, di, dj, dl, n, dO);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dO, n * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// ---------------------------------------------------------------------------------------
// joint path
// ---------------------------------------------------------------------------------------
static CkLayout layout_of(const ck_handle* h) { return CkLayout{h->n[0], h->n0p, h->nend, h->Npad}; }
static bool tables_usable(const ck_handle* h) {
    if (h->exact_cov) return false;
    const int nblk = h->n_procs == 1 ? 1 : 3;
    for (int b = 0; b < nblk; ++b)
        if (!h->tab[b].enabled) return false;
    return true;
}
// The worklist of the next table-path assembly: its counter is zero already -- the exact pass of the previous assembly
// (k_assemble_fix) zeroed it, or the allocation did -- and ITS exact pass will zero the other one.  No memset launch.
static void next_worklist(ck_handle* h) {
    unsigned* cur = h->wl.reset;
    h->wl.reset = h->wl.count;
    h->wl.count = cur;
}

// One assembly, by the tables where they are usable: assemble(fast) launches the assembly kernel; on the table path fix()
// launches the exact pass over the worklist, `fixed` (may be null) is recorded behind it -- the count check that follows is
// host latency -- and a list that overflowed sends the assembly through the exact kernels once more.  Returns 1 where the
// table path finished, 0 where the exact kernels assembled, -1 on an error.
template <class Assemble, class Fix>
static int table_or_exact(ck_handle* h, Assemble assemble, Fix fix, hipEvent_t fixed = nullptr) {
    int table_done = 0;
    for (int attempt = 0; attempt < 2 && !table_done; ++attempt) {
        const bool fast = tables_usable(h) && attempt == 0;
        if (fast) next_worklist(h);   // a zeroed counter, without a memset launch in front of the assembly
        assemble(fast);
        if (!fast) break;
        fix();
        if (fixed) HIPCHK(hipEventRecord(fixed, h->stream));
        unsigned cnt = 0;
        HIPCHK(hipMemcpyAsync(&cnt, h->wl.count, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        h->fallback_total += cnt;
        table_done = cnt <= h->wl.cap;   // else: too many out-of-table pairs for the list -> exact kernels
    }
    HIPCHK(hipGetLastError());
    return table_done;
}

// internal (padded-order) 1-based index -> index in the caller's stacked order
static int64_t external_index(const ck_handle* h, int64_t g) { return g > h->n0p ? g - (h->n0p - h->n[0]) : g; }

// d_noise <- [s d | d] in the internal order (ck_set_noise); needs the layout.  noise_on: some s d > 0
static int ensure_noise(ck_handle* h) {
    if (!h->noise_dirty) return 0;
    h->noise_on = false;
    if (h->noise_var[0].empty() && (h->n_procs < 2 || h->noise_var[1].empty())) {
        h->noise_dirty = false;
        return 0;
    }
    const int64_t Np = h->Npad;
    HIPCHK(h->d_noise.reserve((size_t)(2 * Np)));   // outside the arena, as d_trendX: two rows
    std::vector<double> nv((size_t)(2 * Np), 0.0);
    for (int k = 0; k < h->n_procs && k < 2; ++k) {
        if (h->noise_var[k].empty()) continue;
        const int64_t off = k == 0 ? 0 : h->n0p;
        for (int64_t j = 0; j < h->n[k]; ++j) {
            const double d = h->noise_var[k][(size_t)h->perm[k][(size_t)j]];
            nv[(size_t)(off + j)] = h->noise_scale[k] * d;
            nv[(size_t)(Np + off + j)] = d;
            if (h->noise_scale[k] * d > 0.0) h->noise_on = true;
        }
    }
    HIPCHK(hipMemcpyAsync(h->d_noise, nv.data(), (size_t)(2 * Np) * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->noise_dirty = false;
    return 0;
}
// s d per site for the kernels, or null: no noise set, or all of it zero (the bits of a handle that never saw ck_set_noise)
static const double* noise_sd(const ck_handle* h) { return h->noise_on ? h->d_noise : nullptr; }

extern "C" int ck_assemble_joint(ck_handle* h) {
    CHKH(h);
    if (ensure_layout(h)) return -1;
    if (ensure_noise(h)) return -1;
    h->lik_noise_valid = false;

    HIPCHK(hipEventRecord(h->ev0, h->stream));
    // measurement-error variances on the diagonal, once per assembled Sigma (a second attempt writes every entry anew)
    auto assemble = [&](bool fast) {
        CkPanelMap pm{h->d_tile0, h->d_panel_of, h->d_sigptr, h->n_owned, nullptr, 0, h->d_strip_order};
        ck_launch_assemble_sigma(h->stream, fast, h->d_blk, h->d_tabs, h->d_coefptr, h->metric, h->s0, h->su, layout_of(h), pm,
                                 h->total_tiles, h->wl, fast ? h->assemble_queue : 0);
        if (!fast) ck_launch_assemble_noise(h->stream, h->d_sigptr, noise_sd(h), layout_of(h));
    };
    auto fix = [&] {
        ck_launch_assemble_fix(h->stream, false, h->d_blk, h->metric, 0, nullptr, 0, h->s0, layout_of(h), h->wl, h->d_sigptr, nullptr);
        ck_launch_assemble_noise(h->stream, h->d_sigptr, noise_sd(h), layout_of(h));
    };
    const int fast_done = table_or_exact(h, assemble, fix, h->ev1);   // ev1: table kernel + exact pass
    if (fast_done < 0) return -1;
    HIPCHK(hipMemsetAsync(h->d_info, 0, sizeof(long long), h->stream));
    if (!fast_done) HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(elapsed_ms(h->ev0, h->ev1, &h->t_ms[0]));
    h->assembled = true;
    h->factored = false;
    h->aux_state = AUX_NONE;   // right-hand sides solved with the previous factor are stale from here on
    return 0;
}

extern "C" int ck_num_panels(ck_handle* h, int* n_panels, int* panel_width, int64_t* n_padded) {
    CHKH(h);
    if (ensure_layout(h)) return -1;
    if (n_panels) *n_panels = h->nK;
    if (panel_width) *panel_width = CK_NB;
    if (n_padded) *n_padded = h->Npad;
    return 0;
}

extern "C" int ck_panel_owner(ck_handle* h, int K, int* owner_rank) {
    CHKH(h);
    if (K < 0) return fail("bad panel index");
    *owner_rank = K % h->world;
    return 0;
}

static const double* panel_src(ck_handle* h, int K) {
    return h->sig[K] ? h->sig[K] : (h->recv.empty() ? nullptr : h->recv[(size_t)(K % h->recv_slots)]);
}

extern "C" int ck_panel_buffer(ck_handle* h, int K, void** dev_ptr, int64_t* nbytes) {
    CHKH(h);
    if (ensure_layout(h)) return -1;
    if (K < 0 || K >= h->nK) return fail("bad panel index");
    *dev_ptr = (void*)panel_src(h, K);
    *nbytes = panel_payload(h->Npad, K);
    return 0;
}

static void gemm_timed_begin(ck_handle* h, hipStream_t st = nullptr) {
    if (!st) st = h->stream;
    if (!h->time_gemm) return;
    if (h->gemm_ev_used == h->gemm_ev.size()) {
        EvPair e;
        (void)hipEventCreate(&e.a);
        (void)hipEventCreate(&e.b);
        h->gemm_ev.push_back(e);
    }
    (void)hipEventRecord(h->gemm_ev[h->gemm_ev_used].a, st);
}
static void gemm_timed_end(ck_handle* h, hipStream_t st = nullptr) {
    if (!st) st = h->stream;
    if (!h->time_gemm) return;
    (void)hipEventRecord(h->gemm_ev[h->gemm_ev_used].b, st);
    h->gemm_ev_used++;
}

// sum the event pairs recorded since the last reset into t_ms[slot], t_ms[slot + 1]
// ref != nullptr (the tall sweep: launches of two streams overlap each other): also the UNION of the launches' intervals --
// the time during which the kernel is running at all -- into t_ms[15], from every launch's start / end relative to `ref`
static void gemm_timed_collect(ck_handle* h, int slot, hipEvent_t ref = nullptr) {
    if (!h->time_gemm) return;
    double tot = 0;
    std::vector<std::pair<float, float>> iv;
    for (size_t e = 0; e < h->gemm_ev_used; ++e) {
        tot += elapsed_ms(h->gemm_ev[e].a, h->gemm_ev[e].b);
        if (ref) iv.push_back({(float)elapsed_ms(ref, h->gemm_ev[e].a), (float)elapsed_ms(ref, h->gemm_ev[e].b)});
    }
    h->t_ms[slot] = tot;
    h->t_ms[slot + 1] = (double)h->gemm_ev_used;
    if (ref) {
        std::sort(iv.begin(), iv.end());
        double un = 0, cs = 0, ce = -1;
        for (const auto& x : iv) {
            if (x.first > ce) {
                if (ce >= 0) un += ce - cs;
                cs = x.first;
                ce = x.second;
            } else if (x.second > ce) {
                ce = x.second;
            }
        }
        if (ce >= 0) un += ce - cs;
        h->t_ms[15] = un;
    }
    h->gemm_ev_used = 0;
}

// ---- the building blocks, on an explicit stream --------------------------------------------------
// Sigma update of the block columns J0, J0 + Jstep, ... (nJ of them) by the panels K0 .. K0 + np - 1: the only place this launch
// is written
static void sigma_update_on(ck_handle* h, hipStream_t st, int K0, int np, int J0, int Jstep, int nJ, bool timed) {
    unsigned long long* stamps = nullptr;
    if (h->d_stamps) {   // diagnostic: only launches that fit the stamp buffer are stamped
        const size_t wgs = (size_t)((h->Npad - (int64_t)J0 * CK_NB) / 128) * (CK_NB / 128) * (size_t)nJ;
        if (wgs <= h->n_stamps && (h->stamp_sel == 1 || (nJ > 1 && K0 == h->stamp_sel - 2))) {
            stamps = h->d_stamps;
            h->stamp_grid[0] = (int64_t)ck_tilemap_make(h->nend, J0, Jstep, nJ).total;   // the launch's grid: one row
            h->stamp_grid[1] = 1;
            h->stamp_grid[2] = J0;
            h->stamp_grid[3] = np;
        }
    }
    if (timed) gemm_timed_begin(h, st);
    ck_launch_syrk_group(st, h->d_sigptr, h->d_panelptr, K0, np, J0, Jstep, nJ, h->Npad, h->nend, stamps);
    if (timed) gemm_timed_end(h, st);
}

// two-level panel step on block column K: 8 x (64 x 64 Cholesky, row solves, K = 64 update)
// with_aux (the tall sweep, cooperative panel step only): the right-hand-side rows of block column K walk through the panel as
// further workgroups of the same launch
// split (with_aux only): the cooperative launch on the 512 x 512 head alone, then every row below it and every right-hand-side row
// through k_panel_rows_all -- a chunk below the head spins until the head's chunks have published, and while it spins it holds a
// slot the bulk update running beside the chain would use; k_panel_rows_all's workgroups wait for nobody (same arithmetic per row).
static void panel_factor_on(ck_handle* h, int K, hipStream_t st, bool with_aux = false, bool split = false) {
    double* P = h->sig[K];
    const int64_t R = h->Npad - (int64_t)K * CK_NB;
    double* tail = P + R * CK_NB;   // inverses of the eight diagonal blocks (CK_PANEL_TAIL)
    if (h->panel_fused & 16) {
        // the whole panel step in ONE launch of cooperating workgroups (ck_la.hip: k_panel_coop): a chunk of rows waits for
        // the one chunk above it in the chain instead of for 24 grid-wide launch boundaries
        h->coop_seq += 1;
        int drop = -1;
        if (h->coop_inject_panel == K) {   // test hook (option "coop_inject_panel"): chunk 3 of this panel never publishes, once
            drop = 3;
            h->coop_inject_panel = -1;
        }
        double* X = with_aux ? h->aux + (int64_t)K * h->mpad * CK_NB : nullptr;
        if (split && with_aux && R > CK_NB) {
            ck_launch_panel_coop(st, P, CK_NB, tail, (int64_t)K * CK_NB, h->d_info, h->d_coop, h->coop_seq, h->d_coop + 16, nullptr, 0,
                                 h->coop_spins, drop);
            ck_launch_panel_rows_all(st, P + (int64_t)CK_NB * CK_NB, R - CK_NB, P, tail, X, h->mpad);
            return;
        }
        ck_launch_panel_coop(st, P, R, tail, (int64_t)K * CK_NB, h->d_info, h->d_coop, h->coop_seq, h->d_coop + 16, X, with_aux ? h->mpad : 0,
                             h->coop_spins, drop);
        return;
    }
    if (h->panel_fused & 4) {
        // The 512 x 512 diagonal block first -- right-looking over its eight 64-column sub-blocks, on its own 512
        // rows only (small launches: 64 x 64 Cholesky + inverse, row solves, K = 64 update) -- then every row below
        // it walks through the factored block on its own, in ONE launch (the kernel of the right-hand-side rows):
        // 25 launches per panel, 24 of them on 512 rows, instead of 24 launches over all rows of the panel.
        const int64_t RD = std::min<int64_t>(R, CK_NB);
        for (int q = 0; q < CK_NB / CK_IB; ++q) {
            double* diag = P + (int64_t)q * CK_IB * CK_NB + q * CK_IB;
            double* linv = tail + (int64_t)q * CK_IB * CK_IB;
            ck_launch_potrf64(st, diag, CK_NB, (int64_t)K * CK_NB + q * CK_IB, h->d_info, linv);
            const int64_t r1 = (int64_t)(q + 1) * CK_IB;
            if (RD > r1) ck_launch_trsm64(st, P + r1 * CK_NB + q * CK_IB, CK_NB, RD - r1, linv);
            const int64_t ncols = CK_NB - r1;
            if (ncols > 0 && RD > r1) {
                const int64_t ra = r1 / CK_BM * CK_BM;
                ck_launch_gemm_nt(st, P + ra * CK_NB + r1, CK_NB, P + ra * CK_NB + q * CK_IB, CK_NB,
                                  P + r1 * CK_NB + q * CK_IB, CK_NB, RD - ra, ncols, CK_IB, 1, ra - r1, 1, 0, 0, 0);
            }
        }
        if (R > CK_NB) ck_launch_panel_rows_all(st, P + (int64_t)CK_NB * CK_NB, R - CK_NB, P, tail);
        return;
    }
    if (h->panel_fused & 1) {
        for (int q = 0; q < CK_NB / CK_IB; ++q) {
            double* linv = tail + (int64_t)q * CK_IB * CK_IB;
            ck_launch_panel_diag(st, P, q, (int64_t)K * CK_NB, h->d_info, linv);
            const int64_t r1 = (int64_t)(q + 1) * CK_IB;
            ck_launch_panel_rows(st, P, r1, R - r1, P, q, linv);
        }
        return;
    }
    for (int q = 0; q < CK_NB / CK_IB; ++q) {
        double* diag = P + (int64_t)q * CK_IB * CK_NB + q * CK_IB;
        double* linv = tail + (int64_t)q * CK_IB * CK_IB;
        ck_launch_potrf64(st, diag, CK_NB, (int64_t)K * CK_NB + q * CK_IB, h->d_info, linv);
        const int64_t r1 = (int64_t)(q + 1) * CK_IB;
        ck_launch_trsm64(st, P + r1 * CK_NB + q * CK_IB, CK_NB, R - r1, linv);
        const int64_t ncols = CK_NB - r1;
        if (ncols > 0) {
            const int64_t ra = r1 / CK_BM * CK_BM;   // tile-aligned start row (rows above r1 only touch the unused upper triangle)
            ck_launch_gemm_nt(st, P + ra * CK_NB + r1, CK_NB, P + ra * CK_NB + q * CK_IB, CK_NB,
                              P + r1 * CK_NB + q * CK_IB, CK_NB, R - ra, ncols, CK_IB, 1, ra - r1, 1, 0, 0, 0);
        }
    }
}

// trailing update of the locally owned block columns J in [Jlo, Jhi] by panel K
static void apply_sigma_on(ck_handle* h, int K, const double* P, int Jlo, int Jhi, hipStream_t st, bool timed) {
    int J0 = Jlo;
    while (J0 <= Jhi && (J0 % h->world) != h->rank) ++J0;
    if (J0 > Jhi) return;
    const int nJ = (Jhi - J0) / h->world + 1;
    (void)P;   // the group kernel reads panel K through d_panelptr[K] (own storage or receive buffer)
    sigma_update_on(h, st, K, 1, J0, h->world, nJ, timed);
}

// forward substitution of the right-hand-side rows with the diagonal block of panel K
// Right-hand-side rows that can be nonzero in the columns of panels <= K (a multiple of CK_AUX_ALIGN).  Prediction: all.
// Leave-one-out (ck_loocv): row 0 is dense, row 1 + p starts at column loo_g0 + p -- the rows are sorted by their
// first nonzero column, so the sweep works on a growing prefix (process 0: 58 % of the full sweep's flops,
// process 1: 8 %).
static int64_t aux_rows(const ck_handle* h, int K) {
    if (h->loo_g0 < 0) return h->mpad;
    const int64_t live = (int64_t)(K + 1) * CK_NB - h->loo_g0 + h->loo_dense;   // rows 0 .. live - 1
    return std::min(h->mpad, roundup(std::max<int64_t>(live, 1), CK_AUX_ALIGN));
}

// rows of the right-hand-side block in front of its padding, for the thin last tile row (0: treat every row as live): the
// prediction rows, the data row and the trend rows of a universal call
static int64_t aux_live(const ck_handle* h) { return h->loo_g0 < 0 && h->tall_thin ? h->m + 1 + h->aux_trend : 0; }

// right-hand-side update of the block columns J0 .. J0 + nJ - 1 by the panels K0 .. K0 + np - 1: the only place this launch is
// written
static void aux_group_on(ck_handle* h, hipStream_t st, int K0, int np, int J0, int nJ, bool timed) {
    if (nJ <= 0) return;
    if (timed) gemm_timed_begin(h, st);
    ck_launch_aux_group(st, h->aux, h->mpad, h->d_panelptr, K0, np, J0, nJ, aux_rows(h, K0 + np - 1), h->nend, aux_live(h));
    if (timed) gemm_timed_end(h, st);
}

static void aux_inner_on(ck_handle* h, int K, const double* P, hipStream_t st) {
    double* X = h->aux + (int64_t)K * h->mpad * CK_NB;
    const double* tail = P + (h->Npad - (int64_t)K * CK_NB) * CK_NB;
    const int64_t rows = aux_rows(h, K);
    if (h->panel_fused & 2) {
        ck_launch_panel_rows_all(st, X, rows, P, tail);
        return;
    }
    for (int q = 0; q < CK_NB / CK_IB; ++q) {
        ck_launch_trsm64(st, X + q * CK_IB, CK_NB, rows, tail + (int64_t)q * CK_IB * CK_IB);
        const int64_t r1 = (int64_t)(q + 1) * CK_IB;
        const int64_t ncols = CK_NB - r1;
        if (ncols > 0)
            ck_launch_gemm_nt(st, X + r1, CK_NB, X + q * CK_IB, CK_NB, P + r1 * CK_NB + q * CK_IB, CK_NB, rows,
                              ncols, CK_IB, 0, 0, 1, 0, 0, 0);
    }
}

// aux[J] -= aux[K] * P[(J-K)*NB .., :]^T for J in [Jlo, Jhi], batched over J
static void aux_update_on(ck_handle* h, int K, const double* P, int Jlo, int Jhi, hipStream_t st, bool timed) {
    (void)P;
    // time_gemm 2: only the Sigma updates are timed (one event list per sweep)
    aux_group_on(h, st, K, 1, Jlo, Jhi - Jlo + 1, timed && h->time_gemm == 1);
}

static int ensure_events(ck_handle* h) {
    while ((int)h->ev_col.size() < h->nK + 1) {
        hipEvent_t a, b;
        HIPCHK(hipEventCreateWithFlags(&a, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&b, hipEventDisableTiming));
        h->ev_col.push_back(a);
        h->ev_pan.push_back(b);
    }
    while ((int)h->ev_b2.size() < h->nK + 1) {
        hipEvent_t a;
        HIPCHK(hipEventCreateWithFlags(&a, hipEventDisableTiming));
        h->ev_b2.push_back(a);
    }
    return 0;
}

extern "C" int ck_panel_factor(ck_handle* h, int K) {
    CHKH(h);
    if (!h->assembled) return fail("ck_assemble_joint has not been called");
    if (K < 0 || K >= h->nK) return fail("bad panel index");
    if (!h->sig[K]) return fail("panel " + std::to_string(K) + " is not owned by this rank");
    panel_factor_on(h, K, h->stream);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int ck_panel_apply(ck_handle* h, int K, int what) {
    CHKH(h);
    if (K < 0 || K >= h->nK) return fail("bad panel index");
    const double* P = panel_src(h, K);
    if (what & CK_APPLY_SIGMA) apply_sigma_on(h, K, P, K + 1, h->nK - 1, h->stream, true);
    if ((what & CK_APPLY_AUX) && h->mpad > 0) {
        aux_inner_on(h, K, P, h->stream);
        aux_update_on(h, K, P, K + 1, h->nK - 1, h->stream, true);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int ck_panel_apply_sigma(ck_handle* h, int K, int J_lo, int J_hi) {
    CHKH(h);
    if (K < 0 || K >= h->nK) return fail("bad panel index");
    J_lo = std::max(J_lo, K + 1);
    J_hi = std::min(J_hi, h->nK - 1);
    if (J_lo > J_hi) return 0;
    apply_sigma_on(h, K, panel_src(h, K), J_lo, J_hi, h->stream, true);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int ck_panel_apply_group(ck_handle* h, int K0, int np, int what, int J_lo, int J_hi, int phase, int n_phase) {
    CHKH(h);
    if (K0 < 0 || np < 1 || K0 + np > h->nK) return fail("bad panel group");
    if (n_phase < 1 || phase < 0 || phase >= n_phase) return fail("bad phase");
    for (int p = 0; p < np; ++p)
        if (!panel_src(h, K0 + p)) return fail("panel " + std::to_string(K0 + p) + " is not readable on this rank");
    if (h->world > 1 && np > h->recv_slots) return fail("panel group larger than recv_slots");
    J_lo = std::max(J_lo, K0 + np);
    J_hi = std::min(J_hi, h->nK - 1);
    if (J_lo > J_hi) return 0;
    if (what & CK_APPLY_SIGMA) {
        // the owned block columns of [J_lo, J_hi], every n_phase-th of them starting with the phase-th
        int J0 = J_lo;
        while (J0 <= J_hi && (J0 % h->world) != h->rank) ++J0;
        J0 += phase * h->world;
        if (J0 <= J_hi) {
            const int step = h->world * n_phase;
            const int nJ = (J_hi - J0) / step + 1;
            sigma_update_on(h, h->stream, K0, np, J0, step, nJ, true);
        }
    }
    if ((what & CK_APPLY_AUX) && h->mpad > 0) {
        // right-hand-side block columns: piece `phase` of n_phase contiguous pieces of [J_lo, J_hi]
        const int tot = J_hi - J_lo + 1, per = (tot + n_phase - 1) / n_phase;
        const int a = J_lo + phase * per, b = std::min(J_hi, a + per - 1);
        aux_group_on(h, h->stream, K0, np, a, b - a + 1, h->time_gemm == 1);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int ck_panel_aux_solve(ck_handle* h, int K) {
    CHKH(h);
    if (K < 0 || K >= h->nK) return fail("bad panel index");
    const double* P = panel_src(h, K);
    if (!P) return fail("panel " + std::to_string(K) + " is not readable on this rank");
    if (h->mpad > 0) aux_inner_on(h, K, P, h->stream);
    HIPCHK(hipGetLastError());
    return 0;
}

// The cooperative panel step's error word (d_coop[16]): nonzero when a workgroup of k_panel_coop gave up waiting for a pivot block
// (bounded spin, option "coop_spins": ~2 s; never observed outside the test hook "coop_inject_panel"), which leaves a factor --
// and an info word -- that are not to be trusted.  Read behind a synchronised stream.
static int coop_error(ck_handle* h, unsigned* werr) {
    *werr = 0;
    HIPCHK(hipMemcpy(werr, h->d_coop + 16, sizeof(*werr), hipMemcpyDeviceToHost));
    return 0;
}
// after a timed-out step: clear the word and switch the cooperative step off for this handle; redoing or failing is the caller's
static int coop_switch_off(ck_handle* h) {
    HIPCHK(hipMemset(h->d_coop + 16, 0, sizeof(unsigned)));
    h->panel_fused &= ~16;
    return 0;
}

// the info word alone (ck_factor / ck_factor_predict look at the cooperative step's error word themselves)
static int factor_info_raw(ck_handle* h, int64_t* info) {
    long long v = 0;
    HIPCHK(hipMemcpyAsync(&v, h->d_info, sizeof(v), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *info = external_index(h, (int64_t)v);   // pivots inside the identity padding cannot fail
    return 0;
}

extern "C" int ck_factor_info(ck_handle* h, int64_t* info) {
    CHKH(h);
    long long v = 0;
    HIPCHK(hipMemcpyAsync(&v, h->d_info, sizeof(v), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->panel_fused & 16) {                     // step-wise form: a timed-out cooperative panel step is an error here
        unsigned werr = 0;                         // (ck_factor repeats the factorisation instead)
        if (coop_error(h, &werr)) return -1;
        if (werr != 0) {
            if (coop_switch_off(h)) return -1;
            return fail("cooperative panel step timed out waiting for a pivot block (option panel_fused bit 4 now off): sweep again");
        }
    }
    *info = external_index(h, (int64_t)v);   // pivots inside the identity padding cannot fail
    return 0;
}

// automatic group size (round 4): groups of two pay from 14 panels (scripts/ab_tall.py, N = 10 000: 23.2 -> 22.4 ms), groups of
// four from 40 (3 in rounds 1-3: interleaved A/B at N = 40 000, G = 3 / 4 / 5 / 6 with their best first groups: 491.0 / 488.2 /
// 489.5 / 489.2 ms), 1 below
static int eff_group(const ck_handle* h) { return h->panel_group > 0 ? h->panel_group : (h->nK >= 40 ? 4 : h->nK >= 14 ? 2 : 1); }

// Group boundaries of the single-process sweeps (every form -- ck_factor / ck_predict, the two overlapped sweeps, the tall
// sweep -- takes them from here).  The grouping does not touch the results: an element's updates are accumulated k ascending inside
// a launch and the tile is stored and re-read exactly between launches, so any split performs the same MFMAs per element.
// Groups of G panels; options "group_first" (panels of the FIRST group, 0 = G: a short first group shortens the one chain
// nothing can hide, at the price of one pass over the matrix with a short K) and "group_tail" / "group_tail_panels" (group
// size for the last so-many panels, where a group's updates are shorter than its chain).  starts[g] .. starts[g + 1] - 1.
static std::vector<int> group_plan(const ck_handle* h, int G) {
    std::vector<int> st;
    G = std::max(1, G);
    const int nK = h->nK;
    int K = 0;
    // automatic (-1): from 40 panels on the first group has G / 2 panels -- the one chain nothing can hide under is half as long,
    // for one pass over the matrix with K = 512 G / 2 (G = 4: 489.3 -> 488.2 ms)
    const int gf = h->group_first >= 0 ? h->group_first : (nK >= 40 ? G / 2 : 0);
    if (gf > 0 && gf < G && nK > gf) {
        st.push_back(0);
        K = gf;
    }
    const int tailG = h->group_tail > 0 ? std::min(h->group_tail, G) : G;
    while (K < nK) {
        st.push_back(K);
        K += (nK - K <= h->group_tail_panels) ? tailG : G;
    }
    st.push_back(nK);
    return st;
}

static bool factor_lookahead(const ck_handle* h) {
    if (h->lookahead >= 0) return h->lookahead != 0;
    return (h->panel_fused & 16) && h->panel_group == 0 && h->world == 1 && h->nK >= 12 && h->nK < 64;
}

// ---- the schedules of the single-process sweeps, each written once ------------------------------------
// A sweep is a STEP per panel -- Sigma's panel step, the right-hand-side rows' walk through the panel, or both in one launch --
// and an UPDATE of later block columns by a run of panels, both on an explicit stream: step(st, K) and update(st, K0, np, J0, nJ),
// the block columns J0 .. J0 + nJ - 1 by the panels K0 .. K0 + np - 1.  The four that every form but the tall sweep is made of:
static auto sigma_step(ck_handle* h) {
    return [h](hipStream_t st, int K) { panel_factor_on(h, K, st); };
}
static auto aux_step(ck_handle* h) {
    return [h](hipStream_t st, int K) { aux_inner_on(h, K, h->sig[K], st); };
}
static auto sigma_update(ck_handle* h, bool timed) {
    return [h, timed](hipStream_t st, int K0, int np, int J0, int nJ) { sigma_update_on(h, st, K0, np, J0, 1, nJ, timed); };
}
static auto aux_update(ck_handle* h, bool timed) {
    return [h, timed](hipStream_t st, int K0, int np, int J0, int nJ) { aux_group_on(h, st, K0, np, J0, nJ, timed); };
}

// The chain of one panel group: block column K0 + q first receives the updates of the group's earlier panels in one pass
// (K dimension 512 q), then its step.
template <class Step, class Update>
static void group_chain(hipStream_t st, int K0, int Gc, Step step, Update update) {
    for (int q = 0; q < Gc; ++q) {
        if (q > 0) update(st, K0, q, K0 + q, 1);
        step(st, K0 + q);
    }
}

// One group of the grouped pass on one stream: its chain, then the trailing matrix beyond the group is updated once with
// K = 512 G -- a quarter of the C traffic of G = 1.  chain_done (may be null) is recorded between the two: the group's panels
// are final.
template <class Step, class Update>
static int grouped_pass(ck_handle* h, hipStream_t st, int K0, int Gc, Step step, Update update, hipEvent_t chain_done = nullptr) {
    group_chain(st, K0, Gc, step, update);
    if (chain_done) HIPCHK(hipEventRecord(chain_done, st));
    if (K0 + Gc < h->nK) update(st, K0, Gc, K0 + Gc, h->nK - K0 - Gc);
    return 0;
}

// Look-ahead per panel: as soon as panel K has updated block column K + 1, the step of K + 1 starts on the side stream and runs
// under the update of the columns K + 2.. by panel K.  update(K, Jlo, Jhi, timed): the block columns Jlo .. Jhi by panel K, on
// the handle's own stream.
template <class Step, class Update>
static int panel_lookahead(ck_handle* h, Step step, Update update) {
    if (ensure_events(h)) return -1;
    hipStream_t M = h->stream, S = h->side;
    step(M, 0);
    for (int K = 0; K < h->nK; ++K) {
        if (K > 0) HIPCHK(hipStreamWaitEvent(M, h->ev_pan[K], 0));
        if (K + 1 < h->nK) {
            update(K, K + 1, K + 1, false);
            HIPCHK(hipEventRecord(h->ev_col[K + 1], M));
            HIPCHK(hipStreamWaitEvent(S, h->ev_col[K + 1], 0));
            step(S, K + 1);
            HIPCHK(hipEventRecord(h->ev_pan[K + 1], S));
            update(K, K + 2, h->nK - 1, true);
        }
    }
    return 0;
}

// Look-ahead over panel groups (solve_sweep_la, fused_sweeps_la, tall_sweeps), three streams.  C (the side stream, high priority)
// carries the critical path -- per panel group g its chain and then A(g), the update of the NEXT group's block columns by group g,
// which is all the next chain waits for; T (side_lo) carries the bulk of the trailing updates, B1(g) = group g -> block columns of
// group g + 2 and B2(g) = group g -> everything beyond.  Every block column still receives its updates in the order of the
// sequential sweep (group 0, 1, 2, ... each in one launch with K = 512 G), so the result has the same bits; what changes is that
// the latency-bound chain of group g + 1 runs UNDER the bulk of group g instead of in front of it.
//   C:  chain(g) -> [ev_pan g] -> wait ev_col g - 1 -> A(g) -> chain(g + 1) ...
//   T:  wait ev_pan g -> B1(g) -> [ev_col g] -> B2(g) -> wait ev_pan g + 1 ...
//   M:  wait ev_pan g -> follow(g, K0, Gc), which enqueues that wait itself (fused_sweeps_la: the substitution of group g)
// b2m (option "tall_b2_stream"; never with a follower, whose work M carries): B2(g) on the handle's own stream M instead of behind
// B1(g) on T -- the two only need group g's panels, so the partly filled last round of B1(g) runs beside B2(g)'s tiles instead of
// in front of them.  B1(g) then waits for B2(g - 1), the last writer of its block columns [ev_b2 g - 1]; B2(g) follows B2(g - 1)
// in stream order.
// The callers open the sweep (ev0 on M, C and T wait for it) and close it, each with its own events.
// (an event is always recorded, in host order, before the wait on it is enqueued: a wait on a never-recorded event is a no-op)
template <class Step, class Update, class Follow>
static int group_lookahead(ck_handle* h, const std::vector<int>& gs, bool b2m, Step step, Update update, Follow follow) {
    hipStream_t C = h->side, T = h->side_lo, M = h->stream;
    const int ng = (int)gs.size() - 1;
    auto first = [&](int g) { return gs[(size_t)g]; };
    auto count = [&](int g) { return gs[(size_t)g + 1] - gs[(size_t)g]; };
    for (int g = 0; g < ng; ++g) {
        const int K0 = first(g), Gc = count(g);
        group_chain(C, K0, Gc, step, update);
        HIPCHK(hipEventRecord(h->ev_pan[g], C));   // group g's block columns are final
        if (g + 1 < ng) {
            if (g >= 1) HIPCHK(hipStreamWaitEvent(C, h->ev_col[g - 1], 0));   // B1(g - 1) wrote the same block columns
            update(C, K0, Gc, first(g + 1), count(g + 1));                    // A(g)
        }
        HIPCHK(hipStreamWaitEvent(T, h->ev_pan[g], 0));
        if (g + 2 < ng) {
            if (b2m && g >= 1) HIPCHK(hipStreamWaitEvent(T, h->ev_b2[g - 1], 0));   // B2(g - 1) wrote these block columns last
            update(T, K0, Gc, first(g + 2), count(g + 2));                    // B1(g)
            HIPCHK(hipEventRecord(h->ev_col[g], T));
        }
        if (g + 3 < ng) {
            if (b2m) HIPCHK(hipStreamWaitEvent(M, h->ev_pan[g], 0));
            update(b2m ? M : T, K0, Gc, first(g + 3), h->nK - first(g + 3));   // B2(g)
        }
        if (b2m) HIPCHK(hipEventRecord(h->ev_b2[g], M));
        if (follow(g, K0, Gc)) return -1;
    }
    return 0;
}
static int no_follower(int, int, int) { return 0; }

static int factor_sweep(ck_handle* h) {
    h->gemm_ev_used = 0;
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    if (factor_lookahead(h)) {
        if (panel_lookahead(h, sigma_step(h), [h](int K, int Jlo, int Jhi, bool timed) {
                apply_sigma_on(h, K, h->sig[K], Jlo, Jhi, h->stream, timed);
            }))
            return -1;
        HIPCHK(hipGetLastError());
    } else if (eff_group(h) <= 1) {
        for (int K = 0; K < h->nK; ++K) {
            if (ck_panel_factor(h, K)) return -1;
            if (ck_panel_apply(h, K, CK_APPLY_SIGMA)) return -1;
        }
    } else {
        const std::vector<int> gs = group_plan(h, eff_group(h));
        for (size_t gi = 0; gi + 1 < gs.size(); ++gi)
            if (grouped_pass(h, h->stream, gs[gi], gs[gi + 1] - gs[gi], sigma_step(h), sigma_update(h, true))) return -1;
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    return 0;
}

// The grouped forward sweep with the look-ahead over groups (round 4; ck_predict on a resident factor -- the second field of a
// Predictor, the sites of a new grid): the chain of group g is the one-column in-group updates (280 tiles: they fill 55 % of
// the chip) and the rows' walk through each panel.  Same launches on the same operands in the same order per block column: same bits.
static int solve_sweep_la(ck_handle* h) {
    if (ensure_events(h)) return -1;
    if (!h->side_lo) HIPCHK(hipStreamCreateWithFlags(&h->side_lo, hipStreamNonBlocking));
    hipStream_t C = h->side, T = h->side_lo, M = h->stream;
    const std::vector<int> gs = group_plan(h, eff_group(h));
    HIPCHK(hipEventRecord(h->ev0, M));   // (ev0 / ev1 are free between ck_aux_begin and ck_aux_finish)
    HIPCHK(hipStreamWaitEvent(C, h->ev0, 0));
    HIPCHK(hipStreamWaitEvent(T, h->ev0, 0));
    if (group_lookahead(h, gs, h->tall_b2_stream != 0, aux_step(h), aux_update(h, true), no_follower)) return -1;
    // (ev2 / ev3 are not free: ck_predict_universal and others bracket solve_sweep with them)
    HIPCHK(hipEventRecord(h->ev1, C));
    HIPCHK(hipEventRecord(h->ev_col[(size_t)h->nK], T));   // (ensure_events: nK + 1 entries, the groups use at most nK)
    HIPCHK(hipStreamWaitEvent(M, h->ev1, 0));
    HIPCHK(hipStreamWaitEvent(M, h->ev_col[(size_t)h->nK], 0));
    HIPCHK(hipGetLastError());
    return 0;
}

// forward sweep of the right-hand-side rows through the factor (the L panels are final)
static int solve_sweep(ck_handle* h) {
    const bool la = h->solve_la >= 0 ? h->solve_la != 0 : h->nK >= 40;
    if (la && h->world == 1 && h->loo_g0 < 0 && (h->panel_fused & 2) && eff_group(h) > 1 && h->side) return solve_sweep_la(h);
    if (h->lookahead > 0) {
        if (panel_lookahead(h, aux_step(h), [h](int K, int Jlo, int Jhi, bool timed) {
                aux_update_on(h, K, h->sig[K], Jlo, Jhi, h->stream, timed);
            }))
            return -1;
    } else if (eff_group(h) <= 1) {
        for (int K = 0; K < h->nK; ++K)
            if (ck_panel_apply(h, K, CK_APPLY_AUX)) return -1;
    } else {
        const std::vector<int> gs = group_plan(h, eff_group(h));
        for (size_t gi = 0; gi + 1 < gs.size(); ++gi)
            if (grouped_pass(h, h->stream, gs[gi], gs[gi + 1] - gs[gi], aux_step(h), aux_update(h, true))) return -1;
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// Both sweeps AT ONCE (ck_factor_predict): the factorisation on the high-priority side stream, the forward substitution of
// the right-hand-side rows on the main stream one panel group behind it.  Each sweep alone leaves the chip idle in places
// the other can fill: the panel chain of the factorisation (one launch, ~0.3 ms per panel, a chain of eight 28 us links
// that occupies a handful of CUs), the under-filled in-group launches of the substitution (280 tiles for 512 slots), and
// the drain of every launch (half a tile lifetime on average: ~0.2 ms x 78 launches per sweep).  The sweeps share nothing
// but the L panels, which the substitution reads a group behind their completion (event per group).  Kernels of two
// streams do interleave on this chip while a large grid is being dispatched (ck_debug_stream_overlap: dependent
// side-stream kernels ran, at ~3x their solo latency, under a 32 ms update that they slowed by 1.5 %).
static int fused_sweeps(ck_handle* h) {
    if (ensure_events(h)) return -1;
    if (h->fused_prio == 2 && !h->side_lo) HIPCHK(hipStreamCreateWithFlags(&h->side_lo, hipStreamNonBlocking));
    // option "fused_prio": 0 the factorisation on the high-priority stream | 1 the substitution | 2 neither
    hipStream_t F = h->fused_prio == 0 ? h->side : h->fused_prio == 1 ? h->stream : h->side_lo;
    hipStream_t M = h->fused_prio == 1 ? h->side : h->stream;
    const std::vector<int> gs = group_plan(h, h->fused_group > 0 ? h->fused_group : eff_group(h));
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    if (F != h->stream) HIPCHK(hipStreamWaitEvent(F, h->ev0, 0));
    if (M != h->stream) HIPCHK(hipStreamWaitEvent(M, h->ev0, 0));
    for (int ge = 0; ge + 1 < (int)gs.size(); ++ge) {
        const int K0 = gs[ge], Gc = gs[ge + 1] - gs[ge];
        if (grouped_pass(h, F, K0, Gc, sigma_step(h), sigma_update(h, false), h->ev_pan[ge])) return -1;
        HIPCHK(hipStreamWaitEvent(M, h->ev_pan[ge], 0));
        if (grouped_pass(h, M, K0, Gc, aux_step(h), aux_update(h, false))) return -1;
    }
    HIPCHK(hipEventRecord(h->ev1, F));               // end of the factorisation
    HIPCHK(hipEventRecord(h->ev2, M));               // end of the substitution
    if (F != h->stream) HIPCHK(hipStreamWaitEvent(h->stream, h->ev1, 0));
    if (M != h->stream) HIPCHK(hipStreamWaitEvent(h->stream, h->ev2, 0));
    HIPCHK(hipEventRecord(h->ev3, h->stream));       // end of both
    HIPCHK(hipGetLastError());
    return 0;
}

// The same with a LOOK-AHEAD inside the factorisation (option "fused_la"): group_lookahead on Sigma, and the main stream
// carries the substitution as before, one panel group behind the chain.
static int fused_sweeps_la(ck_handle* h) {
    if (ensure_events(h)) return -1;
    if (!h->side_lo) HIPCHK(hipStreamCreateWithFlags(&h->side_lo, hipStreamNonBlocking));
    hipStream_t C = h->side, T = h->side_lo, M = h->stream;
    const std::vector<int> gs = group_plan(h, h->fused_group > 0 ? h->fused_group : eff_group(h));
    HIPCHK(hipEventRecord(h->ev0, M));
    HIPCHK(hipStreamWaitEvent(C, h->ev0, 0));
    HIPCHK(hipStreamWaitEvent(T, h->ev0, 0));
    auto substitution = [h, M](int g, int K0, int Gc) {
        HIPCHK(hipStreamWaitEvent(M, h->ev_pan[g], 0));
        return grouped_pass(h, M, K0, Gc, aux_step(h), aux_update(h, false));
    };
    if (group_lookahead(h, gs, false, sigma_step(h), sigma_update(h, false), substitution)) return -1;
    HIPCHK(hipEventRecord(h->ev1, C));               // end of the factorisation's chain: the last panel is final
    HIPCHK(hipEventRecord(h->ev2, T));
    HIPCHK(hipStreamWaitEvent(M, h->ev1, 0));
    HIPCHK(hipStreamWaitEvent(M, h->ev2, 0));
    HIPCHK(hipEventRecord(h->ev3, M));               // end of everything
    HIPCHK(hipGetLastError());
    return 0;
}

// ONE sweep over the tall matrix [Sigma; c0^T; z^T] (round 4, option "tall_sweep"): the forward substitution is the panel
// step applied to more rows, so every launch of the factorisation takes the right-hand-side rows along --
// the cooperative panel step as further workgroups (k_panel_coop), the updates as further tiles of the same grid
// (k_tall_group_d) -- instead of a second sweep that shares the chip with the first (fused_sweeps_la: 156 big launches per
// pass on two streams, the substitution's one-column launches filling 280 of 512 slots).  The look-ahead is kept
// (group_lookahead).  Every block column -- of Sigma and of the right-hand-side rows -- receives its updates in the order of
// the sequential sweeps, each in one launch with K = 512 G, and every tile computes what it computed there: same bits as
// ck_factor + ck_predict.
static int tall_sweeps(ck_handle* h) {
    if (ensure_events(h)) return -1;
    if (!h->side_lo) HIPCHK(hipStreamCreateWithFlags(&h->side_lo, hipStreamNonBlocking));
    hipStream_t C = h->side, T = h->side_lo, M = h->stream;
    const std::vector<int> gs = group_plan(h, h->fused_group > 0 ? h->fused_group : eff_group(h));
    HIPCHK(hipEventRecord(h->ev0, M));
    HIPCHK(hipStreamWaitEvent(C, h->ev0, 0));
    HIPCHK(hipStreamWaitEvent(T, h->ev0, 0));
    auto step = [&](hipStream_t st, int K) {
        const int64_t R = h->Npad - (int64_t)K * CK_NB;
        // panel steps that run under a bulk update (behind the first group) and have many chunks: the head cooperatively, the
        // rows on their own
        const bool split = h->tall_split == 1 || (h->tall_split == 2 && K >= gs[1] && R >= h->tall_split_rows);
        panel_factor_on(h, K, st, true, split);
    };
    auto update = [h](hipStream_t st, int K0, int np, int J0, int nJ) {
        if (nJ <= 0) return;
        gemm_timed_begin(h, st);
        ck_launch_tall_group(st, h->d_sigptr, h->aux, h->mpad, K0, np, J0, nJ, h->nend, aux_live(h));
        gemm_timed_end(h, st);
    };
    if (group_lookahead(h, gs, h->tall_b2_stream != 0, step, update, no_follower)) return -1;
    HIPCHK(hipEventRecord(h->ev1, C));               // end of the chain: the last panel is final
    HIPCHK(hipEventRecord(h->ev2, T));
    HIPCHK(hipStreamWaitEvent(M, h->ev1, 0));
    HIPCHK(hipStreamWaitEvent(M, h->ev2, 0));
    HIPCHK(hipEventRecord(h->ev3, M));               // end of everything
    HIPCHK(hipGetLastError());
    return 0;
}

// ck_assemble_joint must have been called; = ck_factor + ck_predict with the two sweeps overlapped.  *info != 0: Sigma is not
// positive definite (pred / pred_err untouched), reported exactly as ck_factor reports it.
extern "C" int ck_factor_predict(ck_handle* h, int i, const double* pcoords, int64_t m, double* pred, double* pred_err,
                                 int64_t* info) {
    CHKH(h);
    if (h->world != 1) return fail("ck_factor_predict is the single-process form");
    if (!h->assembled) return fail("ck_assemble_joint has not been called");
    if (h->factored) return fail("Sigma is already factored; call ck_predict, or ck_assemble_joint again");
    if (!info) return fail("null info");
    // Overlapping pays while a sweep leaves the chip EMPTY for a noticeable share of its time (panel chain, launch drains):
    // 15-20 % at 20 panels, 2-4 % at 79, and at 196 panels (N = 100 000) between +1.5 % and -2 % depending on the device --
    // the launches are long against their drains there, and two kernels sharing the chip cost each other efficiency.
    // Automatic rule (option "fused_sweeps" = -1): overlapped up to 128 panels, one sweep after the other beyond.
    const bool overlap = h->fused_sweeps_opt >= 0 ? h->fused_sweeps_opt != 0 : h->nK <= 128;
    if (!(h->panel_fused & 2) || h->loo_g0 >= 0 || !overlap) {   // (also: options of the A/B scripts) the plain sequence
        h->t_ms[13] = 0.0;   // no overlapped span: ck_timings [1] and [3] are the two sweeps' own times
        if (ck_factor(h, info)) return -1;
        return *info == 0 ? ck_predict(h, i, pcoords, m, pred, pred_err) : 0;
    }
    if (ck_aux_begin(h, i, pcoords, m)) return -1;
    h->gemm_ev_used = 0;
    const bool la = h->fused_la >= 0 ? h->fused_la != 0 : h->nK >= 40;
    const bool tall = (h->panel_fused & 16) && h->tall_sweep != 0;
    if (tall ? tall_sweeps(h) : la ? fused_sweeps_la(h) : fused_sweeps(h)) return -1;
    struct { unsigned werr, pad; long long info; } status = {0u, 0u, 0};   // d_coop[16 .. 19]: the error word and the info word
    HIPCHK(hipMemcpyAsync(&status, h->d_coop + 16, sizeof(status), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *info = external_index(h, (int64_t)status.info);
    const unsigned werr = status.werr;
    if (*info != 0 || werr != 0) {
        // not positive definite, or a cooperative panel step timed out: ck_factor's own handling (redo in the caller's
        // order for numpy's minor index / without the cooperative step), then the substitution on the finished factor.
        // A timed-out step: clear its error word and switch the cooperative step off HERE, so that ck_factor runs the
        // factorisation once, the plain way, instead of repeating a cooperative one and discarding it for the stale flag.
        if (werr != 0 && coop_switch_off(h)) return -1;
        h->gemm_ev_used = 0;
        h->assembled = false;
        h->aux_state = AUX_NONE;
        if (ck_assemble_joint(h)) return -1;
        if (ck_factor(h, info)) return -1;
        if (werr != 0) h->t_ms[12] = 1.0;   // visible in ck_timings: the factorisation was redone
        if (*info != 0) return 0;
        const double redone = h->t_ms[12];
        if (ck_predict(h, i, pcoords, m, pred, pred_err)) return -1;
        h->t_ms[12] = redone;
        return 0;
    }
    h->factored = true;
    HIPCHK(elapsed_ms(h->ev0, h->ev1, &h->t_ms[1]));    // the factorisation's span (it shares the chip with the substitution)
    HIPCHK(elapsed_ms(h->ev0, h->ev3, &h->t_ms[13]));   // both sweeps
    h->t_ms[3] = h->t_ms[13] - h->t_ms[1];   // what the substitution adds behind the factorisation
    h->t_ms[12] = 0.0;
    h->t_ms[5] = h->t_ms[6] = h->t_ms[7] = h->t_ms[8] = 0.0;
    h->t_ms[15] = 0.0;
    if (tall) gemm_timed_collect(h, 5, h->ev0);   // the tall sweep's update launches: sum of their durations and union of their intervals
    else h->gemm_ev_used = 0;
    if (ck_aux_finish(h, pred, pred_err)) return -1;
    h->aux_state = AUX_PREDICT;
    return 0;
}

extern "C" int ck_factor(ck_handle* h, int64_t* info) {
    CHKH(h);
    if (h->world != 1) return fail("ck_factor is the single-process form; drive ck_panel_* for world > 1");
    if (!h->assembled) return fail("ck_assemble_joint has not been called");
    if (h->factored) return fail("Sigma is already factored; call ck_assemble_joint again");
    h->aux_state = AUX_NONE;
    h->t_ms[12] = 0.0;
    if (factor_sweep(h)) return -1;
    {
        // FIRST the cooperative panel step's error word (coop_error): after a timeout the cooperative step is switched off for
        // this handle and the factorisation repeated with one launch per dependency.
        HIPCHK(hipStreamSynchronize(h->stream));
        unsigned werr = 0;
        if (coop_error(h, &werr)) return -1;
        if (werr != 0) {
            if (coop_switch_off(h)) return -1;
            h->assembled = false;
            if (ck_assemble_joint(h)) return -1;
            if (factor_sweep(h)) return -1;
            h->t_ms[12] = 1.0;                  // visible in ck_timings
        }
    }
    if (factor_info_raw(h, info)) return -1;
    if (*info != 0 && h->site_order) {
        // Not positive definite.  numpy names the failing leading minor of Sigma in the CALLER's
        // order (cho_factor, joint_prediction.py:68-69, raises LinAlgError): redo the factorisation in that
        // order so that the reported index is the reference's.  The handle stays in site_order 0.
        h->site_order = 0;
        h->layout_ready = false;
        h->assembled = false;
        if (ck_assemble_joint(h)) return -1;
        if (factor_sweep(h)) return -1;
        if (factor_info_raw(h, info)) return -1;
    }
    HIPCHK(elapsed_ms(h->ev0, h->ev1, &h->t_ms[1]));
    gemm_timed_collect(h, 5);
    h->factored = true;
    return 0;
}

// ---------------------------------------------------------------------------------------
// universal cokriging: the regressors in the internal order (ck_set_trend)
// ---------------------------------------------------------------------------------------
static int trend_total(const ck_handle* h) {
    int p = 0;
    for (int k = 0; k < h->n_procs && k < 2; ++k) p += h->trend_p[k];
    return p;
}

// d_trendX <- the columns of X as rows in the internal order; needs the layout
static int ensure_trend(ck_handle* h) {
    const int p = trend_total(h);
    if (!h->trend_dirty || p == 0) return 0;
    const int64_t Np = h->Npad;
    HIPCHK(h->d_trendX.reserve((size_t)p * Np));   // outside the arena, as d_chunkb: p <= 16 rows
    std::vector<double> xt((size_t)p * Np, 0.0);
    int col = 0;
    for (int k = 0; k < h->n_procs; ++k) {
        const int pk = h->trend_p[k];
        const int64_t nk = h->n[k], off = k == 0 ? 0 : h->n0p;
        for (int64_t j = 0; j < nk; ++j) {
            const int64_t e = h->perm[k][(size_t)j];
            for (int c = 0; c < pk; ++c) xt[(size_t)(col + c) * Np + off + j] = h->trend_F[k][(size_t)(e * pk + c)];
        }
        col += pk;
    }
    HIPCHK(hipMemcpyAsync(h->d_trendX, xt.data(), (size_t)p * Np * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->trend_dirty = false;
    return 0;
}

// rows row0 .. row0 + p - 1 of every right-hand-side panel <- the rows of d_trendX
static int put_trend_rows(ck_handle* h, int64_t row0) {
    const int p = trend_total(h);
    for (int j = 0; j < p; ++j)
        HIPCHK(hipMemcpy2DAsync(h->aux + (row0 + j) * CK_NB, (size_t)h->mpad * CK_NB * 8, h->d_trendX + (int64_t)j * h->Npad,
                                CK_NB * 8, CK_NB * 8, (size_t)h->nK, hipMemcpyDeviceToDevice, h->stream));
    return 0;
}

static int ensure_univ(ck_handle* h, int64_t doubles) {
    HIPCHK(h->d_univ.reserve((size_t)doubles));
    return 0;
}

// the process and its regressor behind column c of X
static std::string trend_column_name(const ck_handle* h, int c) {
    const int k = c < h->trend_p[0] ? 0 : 1;
    return "regressor " + std::to_string(k == 0 ? c : c - h->trend_p[0]) + " of process " + std::to_string(k);
}

// ck_host_gls on (A, b) in the caller's name: a rank-deficient design is refused, naming the process and the regressor
static int trend_gls_solve(const ck_handle* h, const char* name, int p, const double* A, const double* b, double* R, double* beta,
                           double* Ainv, double* logdet, double* bAb) {
    const int bad = ck_host_gls(p, A, b, CK_TREND_TOL, R, beta, Ainv, logdet, bAb);
    if (bad)
        return fail(std::string(name) + ": the trend design is rank deficient: " + trend_column_name(h, bad - 1) +
                    " is, to rounding, a combination of the regressors in front of it (X^T Sigma^-1 X is singular)");
    return 0;
}

// The GLS step behind k_reduce_univ: A = U^T U and b = U^T y from the p trend rows of the reduced rows W (p + 2 doubles each,
// the first trend row at row0), then trend_gls_solve.  A: p x p, kept
// for the caller; the other outputs as ck_host_gls's (any may be null).
static int trend_gls(const ck_handle* h, const char* name, const std::vector<double>& W, int64_t row0, int p, double* A, double* R,
                     double* beta, double* Ainv, double* logdet, double* bAb) {
    std::vector<double> b((size_t)p);
    for (int j = 0; j < p; ++j) {
        const double* wr = &W[(size_t)((row0 + j) * (p + 2))];
        b[(size_t)j] = wr[1];
        for (int l = 0; l < p; ++l) A[(size_t)(j * p + l)] = wr[2 + l];
    }
    return trend_gls_solve(h, name, p, A, b.data(), R, beta, Ainv, logdet, bAb);
}

// ---------------------------------------------------------------------------------------
// the dense predictors' stages: each written once, each hands what it found to its caller -- only the entry points write ck_timings
// ---------------------------------------------------------------------------------------
// Storage of m + 1 + aux_trend right-hand-side rows and of the site arrays that go with them; no device work.  The rows are the
// caller's to fill: aux_begin_impl's prediction sites, or unit_rows' unit vectors.
static int aux_storage(ck_handle* h, int i, int64_t m) {
    if (ensure_layout(h)) return -1;
    if (i < 0 || i >= h->n_procs) return fail("process index out of range");
    if (m < 0) return fail("bad pcoords");
    const int64_t mpad = roundup(m + 1 + h->aux_trend, CK_AUX_ALIGN);
    const int64_t need = mpad * h->Npad;
    if (need > aux_cap(h)) {
        h->aux = nullptr;
        if (dev_alloc(h, h->aux_own, rhs_bytes(mpad, h->Npad))) return -1;
        h->aux = h->aux_own;
    }
    if (mpad > h->p_cap) {
        h->p_cap = 0;   // all four are taken again if one of them fails
        for (auto* b : {&h->p0, &h->d_pcoords, &h->d_pred, &h->pu}) b->reset();
        if (dev_alloc(h, h->p0, site_bytes(mpad)) || dev_alloc(h, h->pu, site_bytes(mpad)) ||
            dev_alloc(h, h->d_pcoords, pair_bytes(mpad)) || dev_alloc(h, h->d_pred, pair_bytes(mpad)))
            return -1;
        h->p_cap = mpad;
    }
    h->p1 = h->p0 + mpad;
    h->p2 = h->p0 + 2 * mpad;
    h->d_err = h->d_pred + mpad;
    h->i_pred = i;
    h->m = m;
    h->mpad = mpad;
    h->aux_state = AUX_NONE;
    h->p_sorted = false;
    return 0;
}

static int aux_assemble_rows(ck_handle* h, const double* xy, int64_t pair_m0, double* k2_ms);

// The assembly stage (K2): the right-hand sides [c0^T; z^T] of m prediction sites of process i, the trend rows X^T behind them
// where aux_trend says so.  *k2_ms: the device milliseconds of the site transform, the table kernel and the exact pass.
static int aux_begin_impl(ck_handle* h, int i, const double* pcoords, int64_t m, double* k2_ms) {
    if (aux_storage(h, i, m)) return -1;
    h->aux_state = AUX_ASSEMBLED;
    // large sets of prediction points are laid out along the Hilbert curve like the data sites
    // (site_order above); ck_aux_finish hands the results back in the caller's order
    std::vector<double> sorted;
    h->p_sorted = h->site_order && m >= 256;
    if (h->p_sorted) {
        double lo[2] = {1e300, 1e300}, hi[2] = {-1e300, -1e300};
        ck_host_bounding_box(pcoords, m, lo, hi);
        ck_host_hilbert_order(pcoords, m, lo, hi, h->pperm);
        sorted.resize((size_t)(2 * m));
        for (int64_t j = 0; j < m; ++j) {
            sorted[2 * j] = pcoords[2 * h->pperm[(size_t)j]];
            sorted[2 * j + 1] = pcoords[2 * h->pperm[(size_t)j] + 1];
        }
        pcoords = sorted.data();   // alive until the event synchronisation at the end of aux_assemble_rows
    }
    return aux_assemble_rows(h, pcoords, -1, k2_ms);
}

// K2's device work on the h->m rows aux_storage laid out, xy (h->m x 2) their coordinates in the internal order.  pair_m0 < 0:
// sites of process h->i_pred.  pair_m0 >= 0 (ck_predict_pair): the stacked rows of both processes (ck_host.h: CkPairPlan; xy has
// zeros in the gap).
static int aux_assemble_rows(ck_handle* h, const double* pcoords, int64_t pair_m0, double* k2_ms) {
    const int i = h->i_pred;
    const int64_t m = h->m, mpad = h->mpad;
    HIPCHK(hipMemsetAsync(h->d_pcoords, 0, 2 * mpad * 8, h->stream));
    if (m > 0) HIPCHK(hipMemcpyAsync(h->d_pcoords, pcoords, 2 * m * 8, hipMemcpyHostToDevice, h->stream));
    // timed like ck_assemble_joint: the device work of K2 (site transform, table kernel, exact pass) -- not the upload of the
    // prediction coordinates in front of it nor the host round trip for the worklist count behind it
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    // table path: ONE launch -- the assembly transforms the prediction sites itself (every strip its 64 rows; the strips of
    // block column 0 store p0 / pu for the exact pass and the later users) and starts on a counter the previous exact pass
    // zeroed.  Round 3 had k_prep_sites, a memset, the assembly and the exact pass: the gaps between the four were a tenth of
    // the stage.  The exact path (no tables) keeps the separate transform.
    const bool fold = tables_usable(h);
    if (!fold) ck_launch_prep_sites(h->stream, h->d_pcoords, mpad, h->metric, h->p0, h->p1, h->p2, h->pu);
    auto assemble = [&](bool fast) {
        ck_launch_assemble_aux(h->stream, fast, h->d_blk, h->d_tabs, h->d_coefptr, h->metric, i, h->p0, h->pu, m, mpad, h->s0, h->su,
                               h->z, layout_of(h), h->nK, h->aux, h->wl, fast && fold ? h->d_pcoords : nullptr,
                               fast ? h->assemble_queue : 0, pair_m0);
    };
    auto fix = [&] {
        ck_launch_assemble_fix(h->stream, true, h->d_blk, h->metric, i, h->p0, mpad, h->s0, layout_of(h), h->wl, h->d_sigptr, h->aux,
                               pair_m0);
    };
    const int fast_done = table_or_exact(h, assemble, fix, h->ev1);
    if (fast_done < 0) return -1;
    if (!fast_done) HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipEventSynchronize(h->ev1));   // pcoords is caller memory: do not return before the copy is done
    HIPCHK(elapsed_ms(h->ev0, h->ev1, k2_ms));
    if (h->aux_trend > 0 && put_trend_rows(h, m + 1)) return -1;   // universal cokriging: X^T behind the data row
    return 0;
}

// The timed sweep stage: the forward sweep over the right-hand sides between ev2 and ev3, the handle's second event pair (ev0 /
// ev1 belong to the stages around it).  The caller reads the window behind its next synchronisation.
static int timed_solve_sweep(ck_handle* h) {
    h->gemm_ev_used = 0;
    HIPCHK(hipEventRecord(h->ev2, h->stream));
    if (solve_sweep(h)) return -1;
    HIPCHK(hipEventRecord(h->ev3, h->stream));
    return 0;
}

extern "C" int ck_aux_begin(ck_handle* h, int i, const double* pcoords, int64_t m) {
    CHKH(h);
    if (m > 0 && !pcoords) return fail("bad pcoords");
    return aux_begin_impl(h, i, pcoords, m, &h->t_ms[2]);
}

extern "C" int ck_aux_finish(ck_handle* h, double* pred, double* pred_err) {
    CHKH(h);
    if (h->mpad <= 0) return fail("ck_aux_begin has not been called");
    if (const char* call = aux_state_text[h->aux_state].call)
        return fail(std::string("ck_aux_finish: the last call was ") + call + "; call ck_aux_begin first");
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    const double c0 = h->blk[2 * h->i_pred].amp + h->blk[2 * h->i_pred].nugget;   // sigma_i^2 + nugget_i (model.py:194-196 at h = 0)
    ck_launch_reduce_pred(h->stream, h->aux, h->mpad, h->nK, h->m, h->m, c0, h->d_pred, h->d_err);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    if (h->m > 0 && !h->p_sorted) {
        HIPCHK(hipMemcpyAsync(pred, h->d_pred, h->m * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(pred_err, h->d_err, h->m * 8, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->time_gemm == 2) gemm_timed_collect(h, 5);   // step-wise form: the Sigma updates of this sweep
    if (h->m > 0 && h->p_sorted) {   // back to the caller's order
        std::vector<double> tp((size_t)h->m), te((size_t)h->m);
        HIPCHK(hipMemcpyAsync(tp.data(), h->d_pred, h->m * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(te.data(), h->d_err, h->m * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        for (int64_t j = 0; j < h->m; ++j) {
            pred[h->pperm[(size_t)j]] = tp[(size_t)j];
            pred_err[h->pperm[(size_t)j]] = te[(size_t)j];
        }
    }
    HIPCHK(elapsed_ms(h->ev0, h->ev1, &h->t_ms[4]));
    return 0;
}

extern "C" int ck_predict(ck_handle* h, int i, const double* pcoords, int64_t m, double* pred, double* pred_err) {
    CHKH(h);
    if (h->world != 1) return fail("ck_predict is the single-process form");
    if (!h->factored) return fail("ck_factor has not been called");
    if (ck_aux_begin(h, i, pcoords, m)) return -1;
    if (timed_solve_sweep(h)) return -1;
    if (ck_aux_finish(h, pred, pred_err)) return -1;
    HIPCHK(elapsed_ms(h->ev2, h->ev3, &h->t_ms[3]));
    gemm_timed_collect(h, 7);
    h->aux_state = AUX_PREDICT;
    return 0;
}

// ---------------------------------------------------------------------------------------
// universal cokriging (ck_predict_universal): GLS trend jointly with the kriging
// ---------------------------------------------------------------------------------------
// The right-hand sides are ck_predict's [c0^T; z^T] with the p trend rows X^T behind the data row; the same sweep carries them
// (a row's result does not depend on its neighbours), so V = L^-1 c0 and y = L^-1 z keep ck_predict's bits.  One pass of
// k_reduce_univ dots every solved row with [y; U]: |V_s|^2, V_s . y, U^T V_s for the sites and, over the trend rows themselves,
// A = U^T U and b = U^T y.  The p x p GLS step runs on the host (ck_host_gls), and so does the O(m p^2) epilogue
// pred_s = V_s . y + r_s^T beta, pred_err_s^2 = c0 - |V_s|^2 + r_s^T A^-1 r_s, r_s = x0_s - U^T V_s.
extern "C" int ck_predict_universal(ck_handle* h, int i, const double* pcoords, int64_t m, const double* f0, double* pred,
                                    double* pred_err, double* beta, double* beta_cov) {
    CHKH(h);
    if (h->world != 1)
        return fail("ck_predict_universal is the single-process form: this handle is partitioned (world = " +
                    std::to_string(h->world) + ")");
    if (!h->factored) return fail("ck_predict_universal: ck_factor has not been called");
    if (i < 0 || i >= h->n_procs) return fail("process index out of range");
    if (m < 0 || (m > 0 && (!pcoords || !pred || !pred_err))) return fail("ck_predict_universal: bad prediction arrays");
    const int p = trend_total(h);
    if (p == 0) return ck_predict(h, i, pcoords, m, pred, pred_err);   // no trend: simple cokriging, ck_predict's bits
    const int pi = h->trend_p[i], offi = i == 0 ? 0 : h->trend_p[0];
    if (m > 0 && pi > 0 && !f0) return fail("ck_predict_universal: null regressors of the prediction sites");
    for (int64_t e = 0; e < m * pi; ++e)
        if (!std::isfinite(f0[e]))
            return fail("ck_predict_universal: regressor " + std::to_string(e % pi) + " is not finite at prediction site " +
                        std::to_string(e / pi));
    const auto t_begin = std::chrono::steady_clock::now();
    timings_from(h, 40);
    if (ensure_trend(h)) return -1;
    CallGuard guard(h, AUX_UNIVERSAL, false);
    h->aux_trend = p;
    static const double no_site[2] = {0.0, 0.0};
    if (aux_begin_impl(h, i, m > 0 ? pcoords : no_site, m, &h->t_ms[40])) return -1;
    if (timed_solve_sweep(h)) return -1;
    const int q = 1 + p;
    const int64_t nrows = m + 1 + p;
    if (ensure_univ(h, nrows * (q + 1))) return -1;
    ck_launch_reduce_univ(h->stream, h->aux, h->mpad, h->nK, nrows, m, q, h->d_univ);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    std::vector<double> W((size_t)(nrows * (q + 1)));
    HIPCHK(hipMemcpyAsync(W.data(), h->d_univ, W.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(elapsed_ms(h->ev2, h->ev3, &h->t_ms[41]));
    HIPCHK(elapsed_ms(h->ev3, h->ev1, &h->t_ms[42]));
    gemm_timed_collect(h, 7);
    // ---- the GLS step
    auto t0 = std::chrono::steady_clock::now();
    std::vector<double> A((size_t)p * p), bh((size_t)p), Ai((size_t)p * p);
    if (trend_gls(h, "ck_predict_universal", W, m + 1, p, A.data(), nullptr, bh.data(), Ai.data(), nullptr, nullptr)) return -1;
    h->t_ms[43] = ms_since(t0);
    const auto t1 = std::chrono::steady_clock::now();
    // ---- the epilogue, in the caller's order
    const double c0 = h->blk[2 * i].amp + h->blk[2 * i].nugget;   // sigma_i^2 + nugget_i, as ck_aux_finish
    ck_host_universal_finish(W.data(), bh.data(), Ai.data(), f0, h->p_sorted ? h->pperm.data() : nullptr, c0, m, p, pi, offi, pred,
                             pred_err);
    if (beta) memcpy(beta, bh.data(), (size_t)p * 8);
    if (beta_cov) memcpy(beta_cov, Ai.data(), (size_t)p * p * 8);
    h->t_ms[44] = ms_since(t1);
    h->t_ms[45] = ms_since(t_begin);
    return 0;
}

// ---------------------------------------------------------------------------------------
// _verify_model (src/joint_prediction.py:60-66, 260-274)
// ---------------------------------------------------------------------------------------
// The reference factorises the stacked (m + N) x (m + N) matrix [[C_pp, c0^T], [c0, Sigma]] and warns when
// that fails.  Sigma is positive definite here (ck_factor succeeded), so the stacked matrix is positive definite
// iff the Schur complement  S = C_pp - c0^T Sigma^-1 c0 = C_pp - V^T V  is, and V^T = (L^-1 c0)^T are exactly the
// solved right-hand-side rows the last ck_predict left on the device: assemble C_pp (the auto-covariance of
// process i at the prediction sites, nugget where h == 0, :94-102) in the packed panel format of Sigma, subtract
// V^T V in one pass over the rows (ck_la.hip: k_schur_syrk_d), and run the same blocked Cholesky on it --
// 2 N m^2 / 2 + m^3 / 3 flop instead of (m + N)^3 / 3.
// the factorisation drivers work on the handle's matrix: point them at the Schur complement for one sweep
struct SchurSwap {
    ck_handle* h;
    std::vector<double*> sig;
    double **d_sigptr, **d_panelptr;
    int nK, time_gemm, world, rank;
    int64_t Npad, nend;
    long long* d_info;
    int lookahead;
    bool assembled;
    explicit SchurSwap(ck_handle* hh, int nJ, int64_t Mp, int64_t m_valid) : h(hh) {
        sig = h->sig;
        d_sigptr = h->d_sigptr;
        d_panelptr = h->d_panelptr;
        nK = h->nK;
        Npad = h->Npad;
        nend = h->nend;
        d_info = h->d_info;
        time_gemm = h->time_gemm;
        lookahead = h->lookahead;
        assembled = h->assembled;
        world = h->world;
        rank = h->rank;
        h->sig = h->sch.sig;
        h->d_sigptr = h->d_panelptr = h->sch.d_ptr;
        h->nK = nJ;
        h->Npad = Mp;
        h->nend = m_valid;
        h->d_info = h->sch.d_info;
        h->time_gemm = 0;
        h->lookahead = 0;
        h->assembled = true;
        h->world = 1;
        h->rank = 0;
    }
    ~SchurSwap() {
        h->sig = sig;
        h->d_sigptr = d_sigptr;
        h->d_panelptr = d_panelptr;
        h->nK = nK;
        h->Npad = Npad;
        h->nend = nend;
        h->d_info = d_info;
        h->time_gemm = time_gemm;
        h->lookahead = lookahead;
        h->assembled = assembled;
        h->world = world;
        h->rank = rank;
    }
};

// The entries (R, C), C <= R < n, of a packed lower triangle panel by panel: one download and one synchronisation per panel
// this process holds, visit(R, C, value) on the host
template <class Visit>
static int read_lower(ck_handle* h, const std::vector<double*>& sig, int nJ, int64_t n, Visit visit) {
    std::vector<double> panel;
    for (int J = 0; J < nJ; ++J) {
        const int64_t R0 = (int64_t)J * CK_NB, rows = n - R0;
        if (!sig[(size_t)J] || rows <= 0) continue;
        panel.resize((size_t)(rows * CK_NB));
        HIPCHK(hipMemcpyAsync(panel.data(), sig[(size_t)J], (size_t)(rows * CK_NB) * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        for (int64_t R = R0; R < n; ++R)
            for (int64_t C = R0; C < std::min<int64_t>(R0 + CK_NB, R + 1); ++C)
                visit(R, C, panel[(size_t)((R - R0) * CK_NB + (C - R0))]);
    }
    return 0;
}

// the Schur complement's packed panels (Mp = roundup(sites, CK_NB) rows, a Sigma-like block-column layout) and the
// assembly state that goes with them; kept between calls with the same padded order
static int schur_ensure(ck_handle* h, int64_t Mp) {
    if (h->sch.M == Mp) return 0;
    const int nJ = (int)(Mp / CK_NB);
    h->sch = {};   // M = 0: a failure below leaves no Schur complement, and the next call starts over
    h->sch.panels.resize((size_t)nJ);
    std::vector<int> tile0, panel_of;
    int acc = 0;
    for (int J = 0; J < nJ; ++J) {
        const int64_t rows = Mp - (int64_t)J * CK_NB;
        HIPCHK(h->sch.panels[(size_t)J].reserve((size_t)(rows * CK_NB + CK_PANEL_TAIL)));
        h->sch.sig.push_back(h->sch.panels[(size_t)J]);
        tile0.push_back(acc);
        panel_of.push_back(J);
        acc += (int)(rows / 64);
    }
    tile0.push_back(acc);
    h->sch.tiles = acc;
    HIPCHK(h->sch.d_ptr.reserve((size_t)nJ));
    HIPCHK(hipMemcpy(h->sch.d_ptr, h->sch.sig.data(), (size_t)nJ * sizeof(double*), hipMemcpyHostToDevice));
    HIPCHK(h->sch.d_tile0.reserve(tile0.size()));
    HIPCHK(h->sch.d_panel_of.reserve(panel_of.size() + 1));
    HIPCHK(hipMemcpy(h->sch.d_tile0, tile0.data(), tile0.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->sch.d_panel_of, panel_of.data(), panel_of.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(h->sch.pc.reserve((size_t)(2 * Mp)));
    HIPCHK(h->sch.c.reserve((size_t)(3 * Mp)));
    HIPCHK(h->sch.u.reserve((size_t)(3 * Mp)));
    HIPCHK(h->sch.d_blk.reserve(3));
    HIPCHK(h->sch.d_tabs.reserve(3));
    HIPCHK(h->sch.d_coefptr.reserve(3));
    HIPCHK(h->sch.d_info.reserve(1));
    h->sch.M = Mp;
    return 0;
}

static int factor_sweep(ck_handle* h);

// S = C_pp - V^T V of the m prediction sites of the last ck_predict in the Schur buffers (schur_ensure(h, Mp) first): C_pp, the
// auto-covariance of process i_pred at the sites (nugget where h == 0), assembled in the packed panel format of Sigma, minus
// V^T V over the solved right-hand-side rows (k_schur_syrk_d).  Consumes the data row m of the right-hand sides.  ms_cpp /
// ms_vtv (may be null): device milliseconds of the assembly and of V^T V.
// pair_m0 >= 0 (ck_conditional_draws_pair): the m rows are ck_predict_pair's stacked sites of both processes -- a two-process
// site set with the layout {pair_m0, roundup(pair_m0, 64), m, Mp} and the model's own three blocks (cross block without nugget);
// the gap rows come out as identity rows, and V^T V leaves them so (their right-hand-side rows are zeros).
static int schur_build(ck_handle* h, double* ms_cpp = nullptr, double* ms_vtv = nullptr, int64_t pair_m0 = -1) {
    const int64_t m = h->m, mpad = h->mpad;
    const int64_t Mp = roundup(m, CK_NB);
    const int nJ = (int)(Mp / CK_NB);
    const bool timed = ms_cpp || ms_vtv;
    // the prediction sites of ONE process as a site set: every tile uses the auto-block (i, i), replicated into all
    // three slots of the block / table arrays
    const int b0 = pair_m0 >= 0 ? 0 : 2 * h->i_pred, b1 = pair_m0 >= 0 ? 1 : b0, b2 = pair_m0 >= 0 ? 2 : b0;
    CkMatern hb[3] = {h->blk[b0], h->blk[b1], h->blk[b2]};
    CkTable ht[3] = {h->tab[b0], h->tab[b1], h->tab[b2]};
    double* hc[3] = {h->d_coef[b0], h->d_coef[b1], h->d_coef[b2]};
    HIPCHK(hipMemcpyAsync(h->sch.d_blk, hb, sizeof(hb), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->sch.d_tabs, ht, sizeof(ht), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->sch.d_coefptr, hc, sizeof(hc), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->sch.pc, 0, (size_t)(2 * Mp) * 8, h->stream));
    HIPCHK(hipMemcpyAsync(h->sch.pc, h->d_pcoords, (size_t)(2 * m) * 8, hipMemcpyDeviceToDevice, h->stream));
    if (timed) HIPCHK(hipEventRecord(h->ev0, h->stream));
    ck_launch_prep_sites(h->stream, h->sch.pc, Mp, h->metric, h->sch.c, h->sch.c + Mp, h->sch.c + 2 * Mp, h->sch.u);
    HIPCHK(hipStreamSynchronize(h->stream));   // hb / ht / hc are stack memory
    const CkLayout L = pair_m0 >= 0 ? CkLayout{pair_m0, roundup(pair_m0, 64), m, Mp} : CkLayout{m, Mp, Mp, Mp};
    auto assemble = [&](bool fast) {
        CkPanelMap pm{h->sch.d_tile0, h->sch.d_panel_of, h->sch.d_ptr, nJ, nullptr, 0, nullptr};
        ck_launch_assemble_sigma(h->stream, fast, h->sch.d_blk, h->sch.d_tabs, h->sch.d_coefptr, h->metric, h->sch.c, h->sch.u, L, pm,
                                 h->sch.tiles, h->wl, fast ? h->assemble_queue : 0);
    };
    auto fix = [&] {
        ck_launch_assemble_fix(h->stream, false, h->sch.d_blk, h->metric, 0, nullptr, 0, h->sch.c, L, h->wl, h->sch.d_ptr, nullptr);
    };
    if (table_or_exact(h, assemble, fix) < 0) return -1;
    if (timed) HIPCHK(hipEventRecord(h->ev1, h->stream));
    // row m of the right-hand sides is y = L^-1 z, not a prediction site (ck_aux_finish has consumed it)
    HIPCHK(hipMemset2DAsync(h->aux + m * CK_NB, (size_t)mpad * CK_NB * 8, 0, (size_t)CK_NB * 8, (size_t)h->nK, h->stream));
    ck_launch_schur_syrk(h->stream, h->sch.d_ptr, h->aux, mpad, h->nK, nJ, Mp);
    HIPCHK(hipGetLastError());
    if (timed) {
        HIPCHK(hipEventRecord(h->ev2, h->stream));
        HIPCHK(hipEventSynchronize(h->ev2));
        double a = 0, b = 0;
        HIPCHK(elapsed_ms(h->ev0, h->ev1, &a));
        HIPCHK(elapsed_ms(h->ev1, h->ev2, &b));
        if (ms_cpp) *ms_cpp = a;
        if (ms_vtv) *ms_vtv = b;
    }
    return 0;
}

// the blocked Cholesky of the Schur buffers (factor_sweep under SchurSwap); *v = 0 or the 1-based failing pivot among the m
// sites in the library's internal order.  again: what the caller should repeat after a cooperative-step timeout.
static int schur_factor(ck_handle* h, long long* v, const char* again) {
    const int64_t m = h->m;
    const int64_t Mp = roundup(m, CK_NB);
    const int nJ = (int)(Mp / CK_NB);
    HIPCHK(hipMemsetAsync(h->sch.d_info, 0, sizeof(long long), h->stream));
    *v = 0;
    SchurSwap swap(h, nJ, Mp, m);
    if (factor_sweep(h)) return -1;   // records ev1 at its end
    HIPCHK(hipMemcpyAsync(v, h->d_info, sizeof(*v), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    unsigned werr = 0;
    if (coop_error(h, &werr)) return -1;
    if (werr != 0) {
        if (coop_switch_off(h)) return -1;
        return fail(std::string("cooperative panel step timed out (option panel_fused bit 4 now off): ") + again);
    }
    return 0;
}

extern "C" int ck_verify_model(ck_handle* h, int64_t* info) {
    CHKH(h);
    if (!info) return fail("null info");
    if (h->world != 1) return fail("ck_verify_model is the single-process form");
    if (const char* call = aux_state_text[h->aux_state].call)
        return fail(std::string("ck_verify_model: the last call was ") + call + ", " + aux_state_text[h->aux_state].clause +
                    "; call ck_predict with the sites to check first");
    if (h->aux_state != AUX_PREDICT) return fail("ck_verify_model needs the solved right-hand sides of a preceding ck_predict");
    const int64_t m = h->m;
    *info = 0;
    if (m <= 0) return 0;
    const int64_t Mp = roundup(m, CK_NB);
    if (schur_ensure(h, Mp)) return -1;
    const auto t_begin = std::chrono::steady_clock::now();
    if (schur_build(h)) return -1;
    long long v = 0;
    if (schur_factor(h, &v, "call ck_predict and ck_verify_model again")) return -1;
    *info = (int64_t)v;   // 1-based index among the prediction sites in the library's internal order, 0 = positive definite
    h->t_ms[11] = ms_since(t_begin);
    return 0;
}

// ---------------------------------------------------------------------------------------
// block (areal) cokriging: weighted sums of the joint point predictor (ck_blocks.hip)
// ---------------------------------------------------------------------------------------
// Block b is the weighted sum of its sites, A[b, a] = w_a.  Its right-hand side is c0_b = sum_a w_a c0(s_a): the point
// rows of K2 are folded into r block rows (k_block_fold), so that the O(N^2) forward sweep runs over r + 1 rows instead of
// m + 1.  pred_b = V_b . y, cov = Cbar - V^T V with Cbar = A C_pp A^T (k_block_prior_part + _sum) -- A S A^T, S the posterior
// covariance of the point predictions.  The sites go through K2 in chunks of option "block_chunk" sites (caller's order),
// each folded into the same block rows: the device memory of the call is bounded by r, not m.

// point the right-hand-side state at the block rows for the sweep (the point rows' buffer stays the handle's)
struct AuxSwap {
    ck_handle* h;
    double* aux;
    int64_t m, mpad;
    bool p_sorted;
    AuxSwap(ck_handle* hh, double* baux, int64_t r, int64_t bmpad) : h(hh), aux(hh->aux), m(hh->m), mpad(hh->mpad), p_sorted(hh->p_sorted) {
        h->aux = baux;
        h->m = r;
        h->mpad = bmpad;
        h->p_sorted = false;
    }
    ~AuxSwap() {
        h->aux = aux;
        h->m = m;
        h->mpad = mpad;
        h->p_sorted = p_sorted;
    }
};

// Slots 0 .. 15 of ck_timings describe the last point-path calls: no stage below writes one, so every return leaves them as they
// were (tests/test_gpu_call_states.py).
extern "C" int ck_predict_blocks(ck_handle* h, int i, const double* pcoords, int64_t m, const int32_t* block,
                                 const double* weight, int32_t r, double* pred, double* pred_err, double* cov) {
    CHKH(h);
    if (h->world != 1) return fail("ck_predict_blocks is the single-process form");
    if (!h->factored) return fail("ck_factor has not been called");
    if (i < 0 || i >= h->n_procs) return fail("process index out of range");
    if (r < 1) return fail("ck_predict_blocks: r must be >= 1");
    if (m < 1 || m > INT32_MAX) return fail("ck_predict_blocks: m must be in [1, 2^31)");
    if (!pcoords || !block || !weight || !pred || !pred_err) return fail("ck_predict_blocks: null argument");
    if (cov && r > 65536) return fail("ck_predict_blocks: the covariance is limited to 65 536 blocks");
    // member lists: off[b] .. off[b + 1], the caller's order inside each block.  The first site at fault is reported, its label
    // before its weight.
    std::vector<int> off;
    std::vector<int64_t> member;
    int64_t q_max = 0, at = 0;
    const int fault = ck_host_block_members(block, m, r, off, member, &q_max, &at);
    for (int64_t a = 0; a < (fault == CK_HOST_BLOCKS_LABEL ? at : m); ++a)
        if (!std::isfinite(weight[a])) return fail("ck_predict_blocks: weight of site " + std::to_string(a) + " is not finite");
    if (fault == CK_HOST_BLOCKS_LABEL)
        return fail("ck_predict_blocks: block label " + std::to_string(block[at]) + " of site " + std::to_string(at) +
                    " is outside [0, r)");
    if (fault == CK_HOST_BLOCKS_EMPTY) return fail("ck_predict_blocks: block " + std::to_string(at) + " has no site");
    const auto t_begin = std::chrono::steady_clock::now();
    // from here on the right-hand sides are block rows (or a chunk's unsolved point rows after a failure)
    CallGuard guard(h, AUX_BLOCKS, true);
    timings_from(h, 16);
    DevTemps tmp;
    // ---- prior of the blocks (diagonal): members in block order, exact-formula coordinates
    std::vector<double> mc((size_t)(2 * m)), mw((size_t)m);
    for (int64_t k = 0; k < m; ++k) {
        const int64_t a = member[(size_t)k];
        mc[2 * (size_t)k] = pcoords[2 * a];
        mc[2 * (size_t)k + 1] = pcoords[2 * a + 1];
        mw[(size_t)k] = weight[a];
    }
    double *d_mc = nullptr, *d_mx = nullptr, *d_mw = nullptr, *d_diag = nullptr, *d_red = nullptr;
    int* d_off = nullptr;
    HIPCHK(tmp.get(&d_mc, (size_t)(2 * m) * 8));
    HIPCHK(tmp.get(&d_mx, (size_t)(3 * m) * 8));
    HIPCHK(tmp.get(&d_mw, (size_t)m * 8));
    HIPCHK(tmp.get(&d_off, ((size_t)r + 1) * sizeof(int)));
    HIPCHK(tmp.get(&d_diag, (size_t)r * 8));
    HIPCHK(tmp.get(&d_red, (size_t)(2 * r) * 8));
    HIPCHK(hipMemcpyAsync(d_mc, mc.data(), (size_t)(2 * m) * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_mw, mw.data(), (size_t)m * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_off, off.data(), ((size_t)r + 1) * sizeof(int), hipMemcpyHostToDevice, h->stream));
    std::vector<long long> poff;
    const int64_t n_pieces = ck_host_prior_pieces(off.data(), r, 0, poff);
    long long* d_poff = nullptr;
    double* d_part = nullptr;
    HIPCHK(tmp.get(&d_poff, poff.size() * sizeof(long long)));
    HIPCHK(tmp.get(&d_part, (size_t)n_pieces * 8));
    HIPCHK(hipMemcpyAsync(d_poff, poff.data(), poff.size() * sizeof(long long), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    ck_launch_prep_sites(h->stream, d_mc, m, h->metric, d_mx, d_mx + m, d_mx + 2 * m, nullptr);
    ck_launch_block_prior(h->stream, h->d_blk + 2 * i, h->metric, d_mx, d_mx + m, d_mx + 2 * m, d_mw, d_off, r, 0, d_poff,
                          n_pieces, d_part, d_diag, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipEventSynchronize(h->ev1));   // mc / mw / off are host memory
    h->t_ms[18] = elapsed_ms(h->ev0, h->ev1);
    // ---- block rows
    const int64_t bmpad = roundup((int64_t)r + 1, CK_AUX_ALIGN);
    if (bmpad * h->Npad > (int64_t)h->baux.cap() && dev_alloc(h, h->baux, rhs_bytes(bmpad, h->Npad))) return -1;
    size_t fr = 0, tot = 0;
    if (h->block_chunk <= 0 && !h->arena) HIPCHK(hipMemGetInfo(&fr, &tot));
    const int64_t chunk = ck_host_block_chunk(h->block_chunk, (int64_t)fr, h->arena ? h->arena_size - h->arena_used : -1,
                                              aux_cap(h) * 8, h->Npad, m);
    int *d_coff = nullptr, *d_crows = nullptr;
    double* d_cw = nullptr;
    HIPCHK(tmp.get(&d_coff, ((size_t)r + 1) * sizeof(int)));
    HIPCHK(tmp.get(&d_crows, (size_t)chunk * sizeof(int)));
    HIPCHK(tmp.get(&d_cw, (size_t)chunk * 8));
    std::vector<int> coff, crows((size_t)chunk), inv((size_t)chunk);
    std::vector<double> cw((size_t)chunk);
    int n_chunks = 0;
    for (int64_t a0 = 0; a0 < m; a0 += chunk, ++n_chunks) {
        const int64_t mc_ = std::min<int64_t>(chunk, m - a0);
        double k2_ms = 0.0;
        if (aux_begin_impl(h, i, pcoords + 2 * a0, mc_, &k2_ms)) return -1;   // K2 on this chunk's sites (synchronised)
        h->aux_state = AUX_BLOCKS;
        h->t_ms[16] += k2_ms;
        // this chunk's member lists (a block may have none here), rows in the library's internal order (Hilbert order when p_sorted)
        for (int64_t j = 0; j < mc_; ++j) inv[(size_t)(h->p_sorted ? h->pperm[(size_t)j] : j)] = (int)j;
        (void)ck_host_block_members(block + a0, mc_, r, coff, member, &q_max, &at);
        for (int64_t k = 0; k < mc_; ++k) {
            crows[(size_t)k] = inv[(size_t)member[(size_t)k]];
            cw[(size_t)k] = weight[a0 + member[(size_t)k]];
        }
        HIPCHK(hipMemcpyAsync(d_coff, coff.data(), ((size_t)r + 1) * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(d_crows, crows.data(), (size_t)mc_ * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(d_cw, cw.data(), (size_t)mc_ * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipEventRecord(h->ev0, h->stream));
        ck_launch_block_fold(h->stream, h->aux, h->mpad, h->nK, h->baux, bmpad, d_coff, d_crows, d_cw, r, mc_, a0 == 0);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->ev1, h->stream));
        HIPCHK(hipEventSynchronize(h->ev1));   // the lists are rewritten for the next chunk
        h->t_ms[17] += elapsed_ms(h->ev0, h->ev1);
    }
    h->t_ms[22] = n_chunks;
    // ---- the forward sweep over the r + 1 block rows on the resident factor, raw reductions V_b . y and |V_b|^2
    {
        AuxSwap swap(h, h->baux, r, bmpad);
        if (timed_solve_sweep(h)) return -1;
        h->gemm_ev_used = 0;
    }
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    ck_launch_reduce_pred(h->stream, h->baux, bmpad, h->nK, r, r, -1.0, d_red, d_red + r);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    std::vector<double> s1((size_t)r), s2((size_t)r), cbar((size_t)r);
    HIPCHK(hipMemcpyAsync(s1.data(), d_red, (size_t)r * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(s2.data(), d_red + r, (size_t)r * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(cbar.data(), d_diag, (size_t)r * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->t_ms[19] = elapsed_ms(h->ev2, h->ev3);
    h->t_ms[20] = elapsed_ms(h->ev0, h->ev1);
    for (int32_t b = 0; b < r; ++b) {
        pred[b] = s1[(size_t)b];
        pred_err[b] = ck_host_err_of(cbar[(size_t)b] - s2[(size_t)b]);
    }
    // ---- the full A S A^T: Cbar's lower triangle in the Schur buffers' packed panels, minus V^T V (k_schur_syrk_d)
    if (cov) {
        const int64_t Mp = roundup(r, CK_NB);
        const int nJ = (int)(Mp / CK_NB);
        if (schur_ensure(h, Mp)) return -1;
        const int64_t n_pieces_full = ck_host_prior_pieces(off.data(), r, 1, poff);
        long long* d_poff_full = nullptr;
        double* d_part_full = nullptr;
        HIPCHK(tmp.get(&d_poff_full, poff.size() * sizeof(long long)));
        HIPCHK(tmp.get(&d_part_full, (size_t)n_pieces_full * 8));
        HIPCHK(hipMemcpyAsync(d_poff_full, poff.data(), poff.size() * sizeof(long long), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipEventRecord(h->ev0, h->stream));
        for (int J = 0; J < nJ; ++J)
            HIPCHK(hipMemsetAsync(h->sch.sig[(size_t)J], 0, (size_t)((Mp - (int64_t)J * CK_NB) * CK_NB) * 8, h->stream));
        ck_launch_block_prior(h->stream, h->d_blk + 2 * i, h->metric, d_mx, d_mx + m, d_mx + 2 * m, d_mw, d_off, r, 1,
                              d_poff_full, n_pieces_full, d_part_full, nullptr, h->sch.d_ptr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->ev1, h->stream));
        ck_launch_schur_syrk(h->stream, h->sch.d_ptr, h->baux, bmpad, h->nK, nJ, Mp);
        HIPCHK(hipGetLastError());
        // rows J NB .. r - 1 of block column J; only R >= C is meaningful
        if (read_lower(h, h->sch.sig, nJ, r, [&](int64_t R, int64_t C, double v) { cov[R * r + C] = cov[C * r + R] = v; })) return -1;
        HIPCHK(hipEventRecord(h->ev2, h->stream));
        HIPCHK(hipEventSynchronize(h->ev2));
        h->t_ms[18] += elapsed_ms(h->ev0, h->ev1);
        h->t_ms[20] += elapsed_ms(h->ev1, h->ev2);
    }
    h->t_ms[21] = ms_since(t_begin);
    return 0;
}

// ---------------------------------------------------------------------------------------
// simulation draw z = L eps  (sim.BivariateRandomField._simulate, src/sim.py:52-54)
// ---------------------------------------------------------------------------------------
extern "C" int ck_sample(ck_handle* h, const double* noise, double* out, int64_t n) {
    CHKH(h);
    if (h->world != 1) return fail("ck_sample is the single-process form");
    if (!h->factored) return fail("ck_factor has not been called");
    if (n != h->N) return fail("n must equal the number of observations");
    if (h->site_order)
        return fail("ck_sample: L eps depends on the order of the sites; set option site_order = 0 before assembling");
    const int64_t Np = h->Npad, n0 = h->n[0], gap = h->n0p - n0;
    std::vector<double> hv(Np, 0.0), ho(Np);
    memcpy(hv.data(), noise, n0 * 8);
    if (n > n0) memcpy(hv.data() + h->n0p, noise + n0, (n - n0) * 8);
    DevTemps tmp;
    double *dv = nullptr, *dout = nullptr;
    HIPCHK(tmp.get(&dv, (size_t)(Np * 8)));
    HIPCHK(tmp.get(&dout, (size_t)(Np * 8)));
    HIPCHK(hipMemcpyAsync(dv, hv.data(), Np * 8, hipMemcpyHostToDevice, h->stream));
    ck_launch_tri_matvec(h->stream, h->d_sigptr, Np, dv, dout);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ho.data(), dout, Np * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(out, ho.data(), n0 * 8);
    if (n > n0) memcpy(out + n0, ho.data() + n0 + gap, (n - n0) * 8);
    return 0;
}

// ---------------------------------------------------------------------------------------
// conditional simulation: draws from the posterior of the joint predictor (ck_draws.hip, ck_la.hip: k_draw_trmm)
// ---------------------------------------------------------------------------------------
// draws[d] = pred + L_S eps_d with S = C_pp - V^T V the posterior covariance of the point predictions (ck_verify_model's
// Schur complement, built by the same code) and L_S its Cholesky factor after deflation: a site whose S_kk is at most
// tol (sigma_i^2 + nugget_i) -- in practice a site on a datum of process i, whose row and column of S vanish -- gets the row
// and column e_k, so that its draw is pred; every other diagonal entry gets jitter (sigma_i^2 + nugget_i).  The noise comes
// from the caller or from the Philox stream of ck_rng.h keyed on (seed, caller's site index, draw index), and the product
// E L_S^T runs on the matrix cores over the lower tiles, in chunks of option "draw_chunk" draws.
// Stages 3 .. 6 on the S that schur_build left in the Schur buffers, for the sites of one process (pair == null: rows == m,
// pc0 their coordinates, c0[0] their prior variance) or for ck_predict_pair's stacked sites (pair: the plan; m = m0 + m1 caller
// columns, rows = pair->rows internal rows with the gap among them, c0[k] the prior variance of process k).  cmap: Mp ints, the
// caller's column of every internal row, -1 where there is none.  tb: the call's first ck_timings slot (the ten slots are laid
// out as ck_conditional_draws').  name: the entry point, for the message of a timed-out cooperative step.
struct DrawSites {
    const CkPairPlan* pair;
    const double *pc0, *pc1;
    int64_t m, rows;
    const std::vector<int>& cmap;
    double c0[2];
};
static int draw_stages(ck_handle* h, const char* name, int tb, const DrawSites& D, int64_t n_draws, uint64_t seed, const double* noise,
                       double tol, double jitter, double* draws, uint8_t* deflated, int64_t* info,
                       std::chrono::steady_clock::time_point t_begin) {
    const int64_t m = D.m, rows = D.rows;
    const int64_t Mp = roundup(rows, CK_NB);
    const int nJ = (int)(Mp / CK_NB);
    const std::vector<int>& cmap = D.cmap;
    // ---- 3. deflation and jitter
    DevTemps tmp;
    unsigned char* d_mask = nullptr;
    int* d_cmap = nullptr;
    double *d_pred = nullptr, *d_ones = nullptr;
    HIPCHK(tmp.get(&d_mask, (size_t)rows));
    HIPCHK(tmp.get(&d_cmap, (size_t)Mp * sizeof(int)));
    HIPCHK(tmp.get(&d_pred, (size_t)Mp * 8));
    HIPCHK(tmp.get(&d_ones, 128 * 8));
    const std::vector<double> ones(128, 1.0);
    HIPCHK(hipMemcpyAsync(d_cmap, cmap.data(), (size_t)Mp * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_ones, ones.data(), 128 * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(d_pred, 0, (size_t)Mp * 8, h->stream));
    HIPCHK(hipMemcpyAsync(d_pred, h->d_pred, (size_t)rows * 8, hipMemcpyDeviceToDevice, h->stream));   // internal order
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    if (D.pair) {
        const double thr[2] = {tol * D.c0[0], tol * D.c0[1]}, jit[2] = {jitter * D.c0[0], jitter * D.c0[1]};
        ck_launch_draw_deflate_pair(h->stream, h->sch.d_ptr, D.pair->m0, D.pair->m0p, rows, thr, jit, d_mask);
    } else {
        ck_launch_draw_deflate(h->stream, h->sch.d_ptr, nJ, rows, tol * D.c0[0], jitter * D.c0[0], d_mask);
    }
    HIPCHK(hipGetLastError());
    std::vector<unsigned char> mask((size_t)rows);
    HIPCHK(hipMemcpyAsync(mask.data(), d_mask, (size_t)rows, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));   // (cmap / ones are host memory)
    int64_t n_defl = 0;
    for (int64_t j = 0; j < rows; ++j) {
        if (cmap[(size_t)j] < 0) continue;   // a gap row of the stacked layout: no site
        deflated[cmap[(size_t)j]] = mask[(size_t)j];
        n_defl += mask[(size_t)j] != 0;
    }
    if (n_defl > 0) ck_launch_draw_zero(h->stream, h->sch.d_ptr, nJ, rows, d_mask);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipEventSynchronize(h->ev1));
    h->t_ms[tb + 3] = elapsed_ms(h->ev0, h->ev1);
    h->t_ms[tb + 8] = (double)n_defl;
    // ---- 4. the factor of S.  Two sites at the same coordinates have identical rows of S: singular unless deflated.  The
    // exact factorisation stops at the later of them (internal order); report that without leaving it to rounding.  (Two
    // PROCESSES at one location are two random variables: S is positive definite there for |rho| < 1.)
    const int64_t stop = D.pair ? ck_host_pair_coincident(*D.pair, D.pc0, D.pc1, mask.data())
                                : ck_host_coincident_site(D.pc0, cmap.data(), mask.data(), m);
    if (stop >= 0) {
        *info = 1 + cmap[(size_t)stop];
        h->t_ms[tb + 7] = ms_since(t_begin);
        return 0;
    }
    {
        long long v = 0;
        HIPCHK(hipEventRecord(h->ev2, h->stream));
        if (schur_factor(h, &v, (std::string("call ") + name + " again").c_str())) return -1;
        HIPCHK(hipEventRecord(h->ev3, h->stream));
        HIPCHK(hipEventSynchronize(h->ev3));
        h->t_ms[tb + 4] = elapsed_ms(h->ev2, h->ev3);
        if (v != 0) {
            *info = 1 + (v - 1 < rows && cmap[(size_t)(v - 1)] >= 0 ? cmap[(size_t)(v - 1)] : (int64_t)(v - 1));
            h->t_ms[tb + 7] = ms_since(t_begin);
            return 0;
        }
    }
    ck_launch_draw_upper(h->stream, h->sch.d_ptr, nJ);
    HIPCHK(hipGetLastError());
    // ---- 5 / 6. noise and the draw product, chunk by chunk
    size_t fr = 0, tot = 0;
    if (h->draw_chunk <= 0) HIPCHK(hipMemGetInfo(&fr, &tot));
    const int64_t chunk = ck_host_draw_chunk(h->draw_chunk, (int64_t)fr, Mp, m, noise != nullptr, n_draws);
    const int64_t ldp = roundup(chunk, 128);
    double *d_E = nullptr, *d_X = nullptr, *d_noise = nullptr;
    HIPCHK(tmp.get(&d_E, (size_t)(ldp * Mp) * 8));
    HIPCHK(tmp.get(&d_X, (size_t)(chunk * m) * 8));
    if (noise) HIPCHK(tmp.get(&d_noise, (size_t)(chunk * m) * 8));
    int n_chunks = 0;
    for (int64_t d0 = 0; d0 < n_draws; d0 += chunk, ++n_chunks) {
        const int64_t nd = std::min<int64_t>(chunk, n_draws - d0);
        if (noise) HIPCHK(hipMemcpyAsync(d_noise, noise + d0 * m, (size_t)(nd * m) * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipEventRecord(h->ev0, h->stream));
        ck_launch_draw_noise(h->stream, d_E, ldp, Mp, nd, rows, d0, d_cmap, d_mask, d_noise, seed, m);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->ev1, h->stream));
        ck_launch_draw_trmm(h->stream, d_X, m, d_E, ldp, nd, h->sch.d_ptr, d_pred, d_ones, d_cmap, rows);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->ev2, h->stream));
        HIPCHK(hipMemcpyAsync(draws + d0 * m, d_X, (size_t)(nd * m) * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        h->t_ms[tb + 5] += elapsed_ms(h->ev0, h->ev1);
        h->t_ms[tb + 6] += elapsed_ms(h->ev1, h->ev2);
    }
    h->t_ms[tb + 9] = n_chunks;
    h->t_ms[tb + 7] = ms_since(t_begin);
    return 0;
}

extern "C" int ck_conditional_draws(ck_handle* h, int i, const double* pcoords, int64_t m, int64_t n_draws, uint64_t seed,
                                    const double* noise, double tol, double jitter, double* draws, double* pred,
                                    double* pred_err, uint8_t* deflated, int64_t* info) {
    CHKH(h);
    if (!pcoords || !draws || !pred || !pred_err || !deflated || !info) return fail("ck_conditional_draws: null argument");
    if (h->world != 1)
        return fail("ck_conditional_draws is the single-process form: this handle is partitioned (world = " +
                    std::to_string(h->world) + ")");
    if (!h->factored) return fail("ck_conditional_draws: ck_factor has not been called");
    if (i < 0 || i >= h->n_procs) return fail("ck_conditional_draws: process index out of range");
    if (m < 1 || m > 65536)
        return fail("ck_conditional_draws: m = " + std::to_string(m) + " prediction sites; the posterior covariance is limited to "
                    "1 .. 65 536 sites");
    if (n_draws < 1) return fail("ck_conditional_draws: n_draws must be >= 1");
    if (!(tol >= 0.0) || !(jitter >= 0.0)) return fail("ck_conditional_draws: tol and jitter must be >= 0");
    const auto t_begin = std::chrono::steady_clock::now();
    const int64_t Mp = roundup(m, CK_NB);
    // device memory: the Schur buffers, the right-hand sides of the point prediction, one chunk of 128 draws
    {
        const int64_t s_bytes = h->sch.M == Mp ? 0 : schur_bytes(Mp);
        const int64_t c_bytes = 128 * (Mp + (noise ? 2 : 1) * m) * 8 + (int64_t)m * 13 + Mp * 12 + 1024;
        CkMemAdmit a;
        if (mem_admit(h, {rhs_bytes(roundup(m + 1, CK_AUX_ALIGN), h->Npad), Mp, 0, c_bytes}, &a)) return -1;
        if (a.need > a.avail)   // (an arena too small for the point rows is ck_predict's to refuse)
            return fail("ck_conditional_draws: needs " + std::to_string(a.need) + " bytes of device memory (" +
                        std::to_string(s_bytes) + " for the posterior covariance of " + std::to_string(m) + " sites, " +
                        std::to_string(c_bytes) + " for a chunk of 128 draws); " + std::to_string(a.avail) + " bytes are available");
    }
    timings_from(h, 30);
    *info = 0;
    // ---- 1. the point prediction (the same call, the same bits)
    {
        const auto t0 = std::chrono::steady_clock::now();
        if (ck_predict(h, i, pcoords, m, pred, pred_err)) return -1;
        h->t_ms[30] = ms_since(t0);
    }
    // ---- 2. S = C_pp - V^T V in the Schur buffers
    if (schur_ensure(h, Mp)) return -1;
    if (schur_build(h, &h->t_ms[31], &h->t_ms[32])) return -1;
    // ---- 3 .. 6. deflation, the factor of S, noise and the draw product
    std::vector<int> cmap((size_t)Mp, -1);
    for (int64_t j = 0; j < m; ++j) cmap[(size_t)j] = (int)(h->p_sorted ? h->pperm[(size_t)j] : j);
    const double c0 = h->blk[2 * i].amp + h->blk[2 * i].nugget;   // sigma_i^2 + nugget_i
    const DrawSites D{nullptr, pcoords, nullptr, m, m, cmap, {c0, c0}};
    return draw_stages(h, "ck_conditional_draws", 30, D, n_draws, seed, noise, tol, jitter, draws, deflated, info, t_begin);
}

// ---------------------------------------------------------------------------------------
// joint prediction and co-simulation of both processes (ck_predict_pair, ck_conditional_draws_pair)
// ---------------------------------------------------------------------------------------
// The sites of both processes ride ONE forward sweep as the stacked right-hand sides [c0(sites of 0)^T; 0; c0(sites of 1)^T; z^T]
// (ck_host.h: CkPairPlan -- the layout of Sigma's own sites, so that a 64-row assembly tile has one process).  A row's result
// does not depend on its neighbours: pred / pred_err are ck_predict's.  The posterior covariance of the stacked sites is S =
// C_pp - V^T V with C_pp = [[C00, C01], [C01^T, C11]]: one entry of its cross block per requested pair (k_pair_cov), all of it
// through schur_build for the draws.
static int pair_admit(const ck_handle* h, const std::string& name, bool null_argument) {
    if (null_argument) return fail(name + ": null argument");
    if (h->world != 1)
        return fail(name + " is the single-process form: this handle is partitioned (world = " + std::to_string(h->world) + ")");
    if (!h->model_set || h->n_procs != 2)
        return fail(name + ": needs a model of two processes (n_procs = " + std::to_string(h->n_procs) + ")");
    if (!h->factored) return fail(name + ": ck_factor has not been called");
    return 0;
}

// K2, the sweep and the reductions of the stacked sites; P: the plan (out).  pred0 / err0: m0 values, pred1 / err1: m1 values, the
// caller's order.  Writes ck_timings [134 .. 137].
static int predict_pair_impl(ck_handle* h, const std::string& name, const double* pc0, int64_t m0, const double* pc1, int64_t m1,
                             double* pred0, double* err0, double* pred1, double* err1, const int64_t* pairs, int64_t q,
                             double* pair_cov, CkPairPlan* P) {
    const auto t_begin = std::chrono::steady_clock::now();
    for (int64_t t = 0; t < q; ++t)
        if (pairs[2 * t] < 0 || pairs[2 * t] >= m0 || pairs[2 * t + 1] < 0 || pairs[2 * t + 1] >= m1)
            return fail(name + ": pair " + std::to_string(t) + " = (" + std::to_string(pairs[2 * t]) + ", " +
                        std::to_string(pairs[2 * t + 1]) + ") is out of range (m0 = " + std::to_string(m0) + ", m1 = " +
                        std::to_string(m1) + ")");
    ck_host_pair_plan(pc0, m0, pc1, m1, h->site_order != 0, P);
    std::vector<int2> prow((size_t)q);
    for (int64_t t = 0; t < q; ++t)
        prow[(size_t)t] = make_int2((int)P->row_of[(size_t)pairs[2 * t]], (int)P->row_of[(size_t)(m0 + pairs[2 * t + 1])]);
    CallGuard guard(h, AUX_PAIR, false);
    const int64_t rows = P->rows;
    if (aux_storage(h, 0, rows)) return -1;
    std::fill(h->t_ms + 134, h->t_ms + 138, 0.0);
    if (aux_assemble_rows(h, P->xy.data(), m0, &h->t_ms[134])) return -1;
    if (timed_solve_sweep(h)) return -1;
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    HIPCHK(hipMemsetAsync(h->d_pred, 0, (size_t)pair_bytes(h->mpad), h->stream));   // (the gap rows have no reduction)
    for (int k = 0; k < 2; ++k) {   // each process's rows with its own prior variance sigma_k^2 + nugget_k
        const int64_t r0 = k == 0 ? 0 : P->m0p;
        ck_launch_reduce_pred(h->stream, h->aux + r0 * CK_NB, h->mpad, h->nK, k == 0 ? m0 : m1, rows - r0,
                              h->blk[2 * k].amp + h->blk[2 * k].nugget, h->d_pred + r0, h->d_err + r0);
    }
    HIPCHK(hipGetLastError());
    DevTemps tmp;
    std::vector<double> tp((size_t)rows), te((size_t)rows);
    if (q > 0) {
        int2* d_rows = nullptr;
        double* d_cov = nullptr;
        HIPCHK(tmp.get(&d_rows, (size_t)q * sizeof(int2)));
        HIPCHK(tmp.get(&d_cov, (size_t)q * 8));
        HIPCHK(hipMemcpyAsync(d_rows, prow.data(), (size_t)q * sizeof(int2), hipMemcpyHostToDevice, h->stream));
        ck_launch_pair_cov(h->stream, h->aux, h->mpad, h->nK, d_rows, q, h->d_blk, h->metric, h->p0, d_cov);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(pair_cov, d_cov, (size_t)q * 8, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    if (rows > 0) {
        HIPCHK(hipMemcpyAsync(tp.data(), h->d_pred, (size_t)rows * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(te.data(), h->d_err, (size_t)rows * 8, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int64_t j = 0; j < rows; ++j) {   // back to the caller's order
        const int c = P->cmap[(size_t)j];
        if (c < 0) continue;
        (c < m0 ? pred0[c] : pred1[c - m0]) = tp[(size_t)j];
        (c < m0 ? err0[c] : err1[c - m0]) = te[(size_t)j];
    }
    HIPCHK(elapsed_ms(h->ev2, h->ev3, &h->t_ms[135]));
    HIPCHK(elapsed_ms(h->ev0, h->ev1, &h->t_ms[136]));
    h->t_ms[137] = ms_since(t_begin);
    return 0;
}

extern "C" int ck_predict_pair(ck_handle* h, const double* pcoords0, int64_t m0, const double* pcoords1, int64_t m1, double* pred0,
                               double* pred_err0, double* pred1, double* pred_err1, const int64_t* pairs, int64_t q,
                               double* pair_cov) {
    CHKH(h);
    if (m0 < 0 || m1 < 0 || q < 0) return fail("ck_predict_pair: m0, m1 and q must be >= 0");
    if (pair_admit(h, "ck_predict_pair",
                   (m0 > 0 && (!pcoords0 || !pred0 || !pred_err0)) || (m1 > 0 && (!pcoords1 || !pred1 || !pred_err1)) ||
                       (q > 0 && pair_cov && !pairs)))
        return -1;
    CkPairPlan P;
    return predict_pair_impl(h, "ck_predict_pair", pcoords0, m0, pcoords1, m1, pred0, pred_err0, pred1, pred_err1, pairs,
                             pair_cov ? q : 0, pair_cov, &P);
}

extern "C" int ck_conditional_draws_pair(ck_handle* h, const double* pcoords0, int64_t m0, const double* pcoords1, int64_t m1,
                                         int64_t n_draws, uint64_t seed, const double* noise, double tol, double jitter,
                                         double* draws, double* pred, double* pred_err, uint8_t* deflated, int64_t* info) {
    CHKH(h);
    const std::string name = "ck_conditional_draws_pair";
    if (m0 < 0 || m1 < 0) return fail(name + ": m0 and m1 must be >= 0");
    if (pair_admit(h, name, (m0 > 0 && !pcoords0) || (m1 > 0 && !pcoords1) || !draws || !pred || !pred_err || !deflated || !info))
        return -1;
    const int64_t m = m0 + m1;
    if (m < 1 || m > 65536)
        return fail(name + ": m0 + m1 = " + std::to_string(m) + " prediction sites; the posterior covariance is limited to "
                    "1 .. 65 536 sites");
    if (n_draws < 1) return fail(name + ": n_draws must be >= 1");
    if (!(tol >= 0.0) || !(jitter >= 0.0)) return fail(name + ": tol and jitter must be >= 0");
    const auto t_begin = std::chrono::steady_clock::now();
    const int64_t rows = roundup(m0, 64) + m1;
    const int64_t Mp = roundup(rows, CK_NB);
    // device memory: the Schur buffers, the right-hand sides of the point prediction, one chunk of 128 draws
    {
        const int64_t s_bytes = h->sch.M == Mp ? 0 : schur_bytes(Mp);
        const int64_t c_bytes = 128 * (Mp + (noise ? 2 : 1) * m) * 8 + rows * 13 + Mp * 12 + 1024;
        CkMemAdmit a;
        if (mem_admit(h, {rhs_bytes(roundup(rows + 1, CK_AUX_ALIGN), h->Npad), Mp, 0, c_bytes}, &a)) return -1;
        if (a.need > a.avail)
            return fail(name + ": needs " + std::to_string(a.need) + " bytes of device memory (" + std::to_string(s_bytes) +
                        " for the posterior covariance of " + std::to_string(m0) + " + " + std::to_string(m1) + " sites, " +
                        std::to_string(c_bytes) + " for a chunk of 128 draws); " + std::to_string(a.avail) + " bytes are available");
    }
    timings_from(h, 124);
    *info = 0;
    // ---- 1. the joint point prediction (ck_predict_pair's stages, the same bits)
    CkPairPlan P;
    {
        const auto t0 = std::chrono::steady_clock::now();
        if (predict_pair_impl(h, name, pcoords0, m0, pcoords1, m1, pred, pred_err, pred + m0, pred_err + m0, nullptr, 0, nullptr, &P))
            return -1;
        h->t_ms[124] = ms_since(t0);
    }
    // ---- 2. S = C_pp - V^T V of the stacked sites in the Schur buffers
    if (schur_ensure(h, Mp)) return -1;
    if (schur_build(h, &h->t_ms[125], &h->t_ms[126], m0)) return -1;
    // ---- 3 .. 6. deflation by each row's own process, the factor of S, noise and the draw product
    std::vector<int> cmap((size_t)Mp, -1);
    std::copy(P.cmap.begin(), P.cmap.end(), cmap.begin());
    const DrawSites D{&P, pcoords0, pcoords1, m, rows, cmap,
                      {h->blk[0].amp + h->blk[0].nugget, h->blk[2].amp + h->blk[2].nugget}};
    return draw_stages(h, name.c_str(), 124, D, n_draws, seed, noise, tol, jitter, draws, deflated, info, t_begin);
}

// ---------------------------------------------------------------------------------------
// batched Cholesky of tiled systems (ck_predict_local's tiled class, ck_cv_folds' big folds)
// ---------------------------------------------------------------------------------------
// The columns [0, cols) of n systems (sys / slab on the device; kq: their padded sizes on the host, largest first, kq_max =
// kq[0]) in groups of G 64-column blocks.  left: the group first receives everything from its left in one pass (K = g0) --
// every tile of a system is read and written once instead of once per earlier group with K = 64 G; else the trailing matrix
// is updated behind every group.  Finished systems drop off the end of the active prefix.
static void factor_tiled_batch(hipStream_t st, const CkLocalSys* sys, double* slab, int n, const int* kq, int cols, int kq_max,
                               int G, bool left, long long* info) {
    int na = n;
    for (int g0 = 0; g0 < cols; g0 += 64 * G) {
        if (left && g0 > 0) ck_launch_local_tiled_left(st, sys, slab, na, g0, 64 * G, kq);
        // the group's diagonal region block by block (diagonal block, then the few chunks of rows inside the region) ...
        for (int b = 0; b < G && g0 + 64 * b < kq_max; ++b) {
            while (na > 0 && kq[na - 1] <= g0 + 64 * b) --na;
            ck_launch_local_tiled_block(st, sys, slab, na, g0, b, kq, info, G);
        }
        // ... then every row below it through all of the group's blocks in one launch
        while (na > 0 && kq[na - 1] <= g0 + 64 * G) --na;
        ck_launch_local_tiled_rows_all(st, sys, slab, na, g0, G, kq);
        if (!left) ck_launch_local_tiled_trailing(st, sys, slab, na, g0, 64 * G, kq);
    }
}

// ---------------------------------------------------------------------------------------
// unit rows as right-hand sides (ck_loocv, ck_cv_folds, ck_loglik / ck_loglik_reml)
// ---------------------------------------------------------------------------------------
// The right-hand sides become row 0 = z, rows 1 .. dense - 1 = the trend rows X^T (REML), row dense + p = the unit vector of
// internal position g0 + p (p < m), and are swept through the factor on the growing prefix of live rows (aux_rows: loo_g0 /
// loo_dense, idle again on every return).  before_sweep (may be null) is recorded between the row fill and the sweep.
static int unit_row_sweep(ck_handle* h, int64_t m, int64_t g0, int dense, hipEvent_t before_sweep) {
    HIPCHK(hipMemsetAsync(h->aux, 0, (size_t)h->mpad * h->Npad * 8, h->stream));
    h->loo_g0 = g0;
    h->loo_dense = dense;
    ck_launch_loo_rows(h->stream, h->aux, h->mpad, m, g0, h->z, h->Npad, dense);
    const int rc = [&]() -> int {
        if (dense > 1 && put_trend_rows(h, 1)) return -1;
        if (before_sweep) HIPCHK(hipEventRecord(before_sweep, h->stream));
        return solve_sweep(h);
    }();
    h->loo_g0 = -1;
    h->loo_dense = 1;
    return rc;
}

// The unit-row stage: storage for the data row, p trend rows and m unit rows from internal position g0 (aux_state <- state),
// their fill and sweep, and the raw reduction of every row -- against y into d_pred / d_err (k_reduce_pred), with trend rows
// against [y; U] into d_univ, p + 2 doubles a row (k_reduce_univ).  The caller's window opens at ev0, in front of the fill
// (from_fill) or between the fill and the sweep; swept (may be null) is recorded between the sweep and the reduction.
static int unit_rows(ck_handle* h, int i, int64_t m, int64_t g0, int p, AuxState state, bool from_fill, hipEvent_t swept) {
    if (aux_storage(h, i, m + p)) return -1;
    h->aux_state = state;
    if (from_fill) HIPCHK(hipEventRecord(h->ev0, h->stream));
    if (unit_row_sweep(h, m, g0, 1 + p, from_fill ? nullptr : h->ev0)) return -1;
    if (swept) HIPCHK(hipEventRecord(swept, h->stream));
    if (p == 0) {
        ck_launch_reduce_pred(h->stream, h->aux, h->mpad, h->nK, m + 1, 0, -1.0, h->d_pred, h->d_err);
    } else {
        const int64_t nrows = m + 1 + p;
        if (ensure_univ(h, nrows * (p + 2))) return -1;
        ck_launch_reduce_univ(h->stream, h->aux, h->mpad, h->nK, nrows, 0, 1 + p, h->d_univ);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------
// leave-one-out cross-validation from ONE factorisation
// ---------------------------------------------------------------------------------------
// The reference re-assembles and re-factorises everything once per withheld datum
// (src/joint_prediction.py:207-257).  Withholding datum q of process i and predicting it from all
// other data is the Gaussian conditional of z_q given z_-q under N(0, Sigma) -- c0 of that
// prediction IS the Sigma column of q (nugget only at h == 0, :112-121) and its prior variance IS
// Sigma_qq -- so
//     pred_q = z_q - (Sigma^-1 z)_q / (Sigma^-1)_qq,      pred_err_q = sqrt(1 / (Sigma^-1)_qq).
// With V = L^-1 E_i (unit vectors of the data of process i as right-hand sides) and y = L^-1 z:
// (Sigma^-1 z)_q = V_q . y and (Sigma^-1)_qq = |V_q|^2: the ordinary forward sweep + reduction.
extern "C" int ck_loocv(ck_handle* h, int i, double* pred, double* pred_err) {
    CHKH(h);
    if (h->world != 1) return fail("ck_loocv is the single-process form");
    if (!h->factored) return fail("ck_factor has not been called");
    if (i < 0 || i >= h->n_procs) return fail("process index out of range");
    const int64_t m = h->n[i];
    if (m <= 0) return 0;
    // storage as for m prediction points; m + 1 rows: row 0 = z, row 1 + q = unit vector of datum q; [ev0, ev1]: the sweep
    if (unit_rows(h, i, m, i == 0 ? 0 : h->n0p, 0, AUX_NONE, false, h->ev1)) return -1;
    std::vector<double> s1(m), s2(m);
    HIPCHK(hipMemcpyAsync(s1.data(), h->d_pred + 1, m * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(s2.data(), h->d_err + 1, m * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(elapsed_ms(h->ev0, h->ev1, &h->t_ms[3]));
    const double* zi = h->h_values[i].data();
    for (int64_t q = 0; q < m; ++q) {   // q: internal position; results go to the caller's index
        const int64_t x = h->perm[i][(size_t)q];
        pred[x] = zi[x] - s1[q] / s2[q];
        pred_err[x] = ck_host_err_of(1.0 / s2[q]);
    }
    return 0;
}

// ---------------------------------------------------------------------------------------
// leave-group-out cross-validation from ONE factorisation
// ---------------------------------------------------------------------------------------
// ck_loocv's identity for a set S of withheld positions (any mix of both processes): with Q = Sigma^-1 and alpha = Sigma^-1 z
//     E[z_S | z_rest] = z_S - Q_SS^-1 alpha_S,      Cov[z_S | z_rest] = Q_SS^-1,
// and with W = the solved unit rows (row of site a = (L^-1 e_a)^T), y = L^-1 z:  Q_SS = W_S W_S^T, alpha_S = W_S y.
//   1. right-hand sides in ck_loocv's layout for the internal positions pmin .. pmax of the withheld data (row 0 = z, row
//      1 + p = unit vector of position pmin + p), swept on the growing prefix of live rows;
//   2. alpha = W y for every row (k_reduce_pred, raw mode) and the folds' Gram matrices on the matrix cores (k_fold_gram: one
//      launch over the tile map of ck_host_fold_plan);
//   3. the fold solves: k_fold_small in LDS for folds of up to 64 members; larger folds as systems of the local predictor's
//      batched Cholesky steps, left-looking, stopped behind the largest fold's last column (ck_folds.hip).
static_assert(CK_FOLD_MAX == CK_HOST_FOLD_MAX, "include/cokrige.h and ck_host.h disagree about the largest fold");
extern "C" int ck_cv_folds(ck_handle* h, int i, const int32_t* fold0, const int32_t* fold1, int32_t n_folds, double* pred,
                           double* pred_err, double* fold_stats, int64_t* info) {
    CHKH(h);
    if (h->world != 1) return fail("ck_cv_folds is the single-process form: this handle is partitioned (world = " + std::to_string(h->world) + ")");
    if (!h->factored) return fail("ck_cv_folds: ck_factor has not been called");
    if (i < 0 || i >= h->n_procs) return fail("ck_cv_folds: process index out of range");
    if (!pred || !pred_err || !info) return fail("ck_cv_folds: null argument");
    const auto t_begin = std::chrono::steady_clock::now();
    if (!(i == 0 ? fold0 : fold1))
        return fail("ck_cv_folds: the fold labels of the predicted process " + std::to_string(i) + " are null");
    CkFoldPlan plan;
    if (ck_host_fold_plan(i, h->n_procs, h->n, h->n0p, h->perm[0].data(), h->n_procs == 2 ? h->perm[1].data() : nullptr, fold0, fold1,
                          n_folds, CK_FOLD_MAX, &plan))
        return -1;
    const int64_t ni = h->n[i];
    const int64_t Np = h->Npad;
    const int64_t m = plan.pmax - plan.pmin + 1;   // unit rows: every internal position from the first withheld one to the last
    const int64_t mpad_need = roundup(m + 1 + h->aux_trend, CK_AUX_ALIGN);
    if (mpad_need * CK_NB * 8 >= (1LL << 31))
        return fail("ck_cv_folds: " + std::to_string(m) + " unit rows are too many for the Gram kernel's 32-bit row offsets (at most " +
                    std::to_string((1LL << 31) / (CK_NB * 8) - CK_AUX_ALIGN) + ")");
    const int64_t ng = (int64_t)plan.gpos.size();
    const int nbig = (int)plan.big.size();
    // Everything of the call besides the right-hand sides is carved from the handle's scratch slab (the one ck_predict_local
    // keeps between calls): the folds' Gram matrices and systems first, then the outputs and the index tables.
    int64_t slab_bytes = 0;
    auto carve = [&](size_t bytes) {
        const int64_t at = slab_bytes;
        slab_bytes += (int64_t)((bytes + 255) / 256 * 256);
        return at;
    };
    const int64_t buf_bytes = plan.buffer_doubles * 8;
    const int64_t o_buf = carve((size_t)buf_bytes), o_x = carve((size_t)ng * 8), o_d = carve((size_t)ng * 8),
                  o_stat = carve((size_t)n_folds * 16), o_linfo = carve((size_t)nbig * sizeof(long long)),
                  o_tiles = carve(plan.tiles.size() * sizeof(CkFoldTile)), o_small = carve(plan.small.size() * sizeof(CkFoldSmall)),
                  o_big = carve((size_t)nbig * sizeof(CkFoldBig)), o_sys = carve((size_t)nbig * sizeof(CkLocalSys)),
                  o_grow = carve((size_t)ng * sizeof(int)), o_fail = carve((size_t)n_folds * sizeof(int));
    const long long slab_doubles = slab_bytes / 8;
    {   // device memory: the right-hand sides and the slab, as far as they have to grow
        const int64_t aux_bytes = rhs_bytes(mpad_need, Np);
        const bool grow = aux_bytes > aux_cap(h) * 8;
        CkMemAdmit a;
        if (mem_admit(h, {aux_bytes, 0, slab_bytes, 0}, &a)) return -1;
        if (a.arena_short)
            return fail("ck_cv_folds needs " + std::to_string(aux_bytes) + " bytes of the arena for its " + std::to_string(m + 1) +
                        " right-hand-side rows of " + std::to_string(Np) + " doubles; " + std::to_string(h->arena_size - h->arena_used) +
                        " bytes are left");
        if (a.need > a.avail)
            return fail("ck_cv_folds needs " + std::to_string(a.need) + " bytes of device memory (" + std::to_string(grow ? aux_bytes : 0) +
                        " for " + std::to_string(m + 1) + " right-hand-side rows of " + std::to_string(Np) + " doubles, " +
                        std::to_string(buf_bytes) + " for the Gram matrices and systems of " + std::to_string(n_folds) + " folds, " +
                        std::to_string(slab_bytes - buf_bytes) + " for their outputs and index tables); " + std::to_string(a.avail) +
                        " bytes are available");
    }
    *info = 0;
    for (int64_t a = 0; a < ni; ++a) pred[a] = pred_err[a] = NAN;
    timings_from(h, 56);
    CallGuard guard(h, AUX_FOLDS, false);
    // outside the timed stages: only the first call of a layout allocates
    if (slab_doubles > local_slab_doubles(h)) HIPCHK(h->local_slab.reserve((size_t)slab_doubles));
    // ---- 1. rows and sweep [ev0, ev1]; 2. alpha (the stage's reduction) and the Gram matrices
    if (unit_rows(h, i, m, plan.pmin, 0, AUX_FOLDS, true, h->ev1)) return -1;
    std::vector<int> grow((size_t)ng);
    for (int64_t g = 0; g < ng; ++g) grow[(size_t)g] = (int)(1 + plan.gpos[(size_t)g] - plan.pmin);
    std::vector<CkLocalSys> sysv((size_t)nbig);
    std::vector<int> kqv((size_t)nbig);
    for (int y = 0; y < nbig; ++y) {
        const CkFoldBig& b = plan.big[(size_t)y];
        sysv[(size_t)y] = CkLocalSys{b.off, b.s, b.kq, b.ld, b.gbase};
        kqv[(size_t)y] = b.kq;
    }
    char* const slab = (char*)h->local_slab.get();
    double *d_buf = (double*)(slab + o_buf), *d_x = (double*)(slab + o_x), *d_d = (double*)(slab + o_d),
           *d_stat = (double*)(slab + o_stat);
    long long* d_linfo = (long long*)(slab + o_linfo);
    CkFoldTile* d_tiles = (CkFoldTile*)(slab + o_tiles);
    CkFoldSmall* d_small = (CkFoldSmall*)(slab + o_small);
    CkFoldBig* d_big = (CkFoldBig*)(slab + o_big);
    CkLocalSys* d_sys = (CkLocalSys*)(slab + o_sys);
    int *d_grow = (int*)(slab + o_grow), *d_fail = (int*)(slab + o_fail);
    HIPCHK(hipMemcpyAsync(d_grow, grow.data(), (size_t)ng * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_tiles, plan.tiles.data(), plan.tiles.size() * sizeof(CkFoldTile), hipMemcpyHostToDevice, h->stream));
    if (!plan.small.empty())
        HIPCHK(hipMemcpyAsync(d_small, plan.small.data(), plan.small.size() * sizeof(CkFoldSmall), hipMemcpyHostToDevice, h->stream));
    if (nbig > 0) {
        HIPCHK(hipMemcpyAsync(d_big, plan.big.data(), (size_t)nbig * sizeof(CkFoldBig), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(d_sys, sysv.data(), (size_t)nbig * sizeof(CkLocalSys), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemsetAsync(d_linfo, 0, (size_t)nbig * sizeof(long long), h->stream));
    }
    ck_launch_fold_gram(h->stream, h->aux, h->mpad, h->nK, d_tiles, (int64_t)plan.tiles.size(), d_grow, d_buf);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev2, h->stream));
    // ---- 3. the fold solves
    ck_launch_fold_small(h->stream, d_small, (int64_t)plan.small.size(), d_buf, d_grow, h->d_pred, d_x, d_d, d_stat, d_fail);
    if (nbig > 0) {
        const int kq_max = plan.big[0].kq, s_max = plan.big[0].s;
        ck_launch_fold_big_fill(h->stream, d_big, nbig, kq_max, d_buf, d_grow, h->d_pred);
        // left-looking in groups of 4 blocks, stopped behind the largest fold's last column
        factor_tiled_batch(h->stream, d_sys, d_buf, nbig, kqv.data(), s_max, kq_max, 4, true, d_linfo);
        ck_launch_fold_big_reduce(h->stream, d_big, nbig, s_max, d_buf, d_linfo, d_x, d_d, d_stat, d_fail);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev3, h->stream));
    std::vector<double> xs((size_t)ng), ds((size_t)ng), st((size_t)n_folds * 2);
    std::vector<int> fl((size_t)n_folds);
    HIPCHK(hipMemcpyAsync(xs.data(), d_x, (size_t)ng * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(ds.data(), d_d, (size_t)ng * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(st.data(), d_stat, (size_t)n_folds * 16, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(fl.data(), d_fail, (size_t)n_folds * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->t_ms[56] = elapsed_ms(h->ev0, h->ev1);
    h->t_ms[57] = elapsed_ms(h->ev1, h->ev2);
    h->t_ms[58] = elapsed_ms(h->ev2, h->ev3);
    const double* zi = h->h_values[i].data();
    for (int32_t f = 0; f < n_folds; ++f) {
        const int s = plan.off[(size_t)f + 1] - plan.off[(size_t)f];
        const bool bad = fl[(size_t)f] != 0;
        if (bad && *info == 0) *info = 1 + f;
        if (fold_stats) {
            fold_stats[3 * f] = (double)s;
            fold_stats[3 * f + 1] = bad ? NAN : st[(size_t)2 * f];
            fold_stats[3 * f + 2] = bad ? NAN : st[(size_t)2 * f + 1];
        }
        if (bad) continue;
        for (int q = 0; q < s; ++q) {
            const int64_t x = plan.cidx[(size_t)(plan.off[(size_t)f] + q)];
            if (x < 0) continue;   // a datum of the other process: withheld, not predicted
            const int64_t g = plan.gbase[(size_t)f] + q;
            pred[x] = zi[x] - xs[(size_t)g];
            pred_err[x] = ck_host_err_of(ds[(size_t)g]);
        }
    }
    h->t_ms[59] = ms_since(t_begin);
    return 0;
}

// ---------------------------------------------------------------------------------------
// Gaussian log-likelihood of the joint model and its gradient (ck_lik.hip)
// ---------------------------------------------------------------------------------------
// The predictor's computation read the other way round: with Sigma = L L^T resident,
//   log|Sigma| = 2 sum log L_qq (k_lik_logdet), z^T Sigma^-1 z = |y|^2, y = L^-1 z: the data row of a one-row sweep.
// The gradient needs G = alpha alpha^T - Sigma^-1.  The right-hand sides are the leave-one-out layout of ck_loocv extended to
// the unit vectors of ALL Npad internal positions (row 0 = z, row 1 + p = e_p; padding positions solve to themselves), swept
// through the factor on the growing prefix of live rows (aux_rows); then alpha_p = W_p . y (k_reduce_pred, raw mode),
// G = alpha alpha^T - W^T W on the lower tiles with the structurally zero panels skipped (ck_la.hip: k_ginv_syrk_d, N^3 / 3
// flop), and one pass of k_loglik_grad over G.  The handle's own state: the factor stays resident; the right-hand sides are
// not prediction rows (AUX_LOGLIK: ck_verify_model / ck_aux_finish refuse until the next ck_predict / ck_aux_begin).
//
// REML (ck_loglik_reml, p = the trend columns of ck_set_trend): the right-hand sides are [z^T; X^T; unit rows], the unit rows
// behind the p trend rows (loo_dense = 1 + p).  k_reduce_univ dots every row with [y; U]: |y|^2, b = U^T y and A = U^T U over
// the first 1 + p rows, alpha_q = W_q . y and B_q = U^T W_q (= (Sigma^-1 X)_q) over the unit rows.  The host forms beta, log|A|,
// b^T A^-1 b, alpha_R = alpha - B beta and C = B R^-T (A = R R^T); k_ginv_syrk_d starts from the rank-(1 + p) term
// alpha_R alpha_R^T + C C^T.  p = 0 is ck_loglik's path, bit for bit.
// ck_loglik_fisher: the same sweep and reductions, but G starts from zero (G = -Sigma^-1) and no contraction follows.
//
// Every stage below is written once and hands what it found to its caller; nothing of a sweep stays on the handle.  The three
// entry points chain the stages and are the only writers of ck_timings [24 .. 29] and [64 .. 69].
static int lik_admit(const ck_handle* h, const char* name, bool null_argument) {
    if (null_argument) return fail(std::string(name) + ": null argument");
    if (h->world != 1)
        return fail(std::string(name) + " is the single-process form: this handle is partitioned (world = " + std::to_string(h->world) +
                    "); the multi-GPU likelihood is not available");
    if (!h->assembled) return fail(std::string(name) + ": ck_assemble_joint has not been called");
    return 0;
}

// Device memory of the unit-row sweep and G, in front of the first allocation: Npad + 1 + p unit / data / trend rows of Npad
// doubles (the right-hand sides) and the Schur buffers of order Npad, as far as they have to grow.  An arena without room for
// the rows is refused here; the caller compares a->need with a->avail and words that refusal.
static int lik_mem_admit(const ck_handle* h, const char* name, int p, CkMemAdmit* a) {
    const int64_t Np = h->Npad, aux_bytes = rhs_bytes(roundup(Np + 1 + p, CK_AUX_ALIGN), Np);
    if (mem_admit(h, {aux_bytes, Np, 0, 0}, a)) return -1;
    if (a->arena_short)
        return fail(std::string(name) + ": the gradient needs " + std::to_string(aux_bytes) + " bytes of the arena for its " +
                    std::to_string(Np + 1 + p) + " right-hand-side rows of " + std::to_string(Np) + " doubles; " +
                    std::to_string(h->arena_size - h->arena_used) + " bytes are left");
    return 0;
}

// What the factor, the sweep and its reductions found.  info != 0: Sigma is not positive definite, the handle has to be
// assembled again, and nothing else is set.
struct LikSweep {
    int64_t info = 0;
    bool factored_here = false;   // ck_factor ran (its milliseconds: ck_timings [1])
    double logdet = 0.0, logdetA = 0.0, quad = 0.0;   // log|Sigma|, log|A| (REML), z^T Sigma^-1 z (REML: z^T P z)
    double sweep_ms = 0.0;                            // sweep and reductions on the device
    std::vector<double> W;            // REML: the reduced rows (k_reduce_univ), 2 + p doubles each
    std::vector<double> beta, R, A;   // REML: the GLS step (A = X^T Sigma^-1 X = R R^T)
    std::vector<double> H;            // REML, on request: Sigma^-1 X (Npad x p)
};

// The factor (here, or the resident one of a preceding ck_factor), the right-hand sides -- row 0 = z, rows 1 .. p = X^T (REML),
// with want_rows the unit vectors of every internal position behind them -- their sweep, the reductions and the GLS step.
static int lik_sweep(ck_handle* h, DevTemps& tmp, const char* name, bool want_rows, int p, bool want_H, LikSweep* S) {
    *S = LikSweep();
    S->factored_here = !h->factored;
    if (S->factored_here ? ck_factor(h, &S->info) : factor_info_raw(h, &S->info)) return -1;
    if (S->info != 0) {   // not positive definite: the factor is unusable; assemble again before the next call
        h->factored = false;
        h->assembled = false;
        return 0;
    }
    const int64_t Np = h->Npad, mrows = want_rows ? Np : 0;
    const int q = 1 + p;
    const CkLayout L = layout_of(h);
    if (p > 0 && ensure_trend(h)) return -1;
    // alpha_p = W_p . y (d_pred[1 + p]) and |y|^2 (d_pred[0]); with a trend every row's dots with [y; U]; log L_qq per panel
    if (unit_rows(h, 0, mrows, 0, p, AUX_LOGLIK, true, nullptr)) return -1;
    const int64_t nrows = mrows + 1 + p;
    double* d_ldp = nullptr;
    HIPCHK(tmp.get(&d_ldp, (size_t)h->nK * 8));
    ck_launch_lik_logdet(h->stream, h->d_sigptr, h->nK, L, d_ldp);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    std::vector<double> ldp((size_t)h->nK);
    HIPCHK(hipMemcpyAsync(ldp.data(), d_ldp, (size_t)h->nK * 8, hipMemcpyDeviceToHost, h->stream));
    if (p == 0) {
        HIPCHK(hipMemcpyAsync(&S->quad, h->d_pred, 8, hipMemcpyDeviceToHost, h->stream));
    } else {
        S->W.resize((size_t)(nrows * (q + 1)));
        HIPCHK(hipMemcpyAsync(S->W.data(), h->d_univ, S->W.size() * 8, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    S->sweep_ms = elapsed_ms(h->ev0, h->ev1);
    double half_logdet = 0.0;
    for (int K = 0; K < h->nK; ++K) half_logdet += ldp[(size_t)K];
    S->logdet = 2.0 * half_logdet;
    if (p > 0) {
        const std::vector<double>& W = S->W;
        S->A.resize((size_t)p * p), S->R.resize((size_t)p * p), S->beta.resize((size_t)p);
        double bAb = 0.0;
        if (trend_gls(h, name, W, 1, p, S->A.data(), S->R.data(), S->beta.data(), nullptr, &S->logdetA, &bAb)) return -1;
        S->quad = W[1] - bAb;   // z^T P z = |y|^2 - b^T A^-1 b
        if (want_H) {
            S->H.assign((size_t)(Np * p), 0.0);
            for (int64_t r = 0; r < mrows; ++r)
                for (int j = 0; j < p; ++j) S->H[(size_t)(r * p + j)] = W[(size_t)((q + r) * (q + 1) + 2 + j)];
        }
    }
    return 0;
}

// G <- start start^T - Sigma^-1 on the lower tiles of the first nend rows, in the Schur buffers (k_ginv_syrk_d over the swept
// unit rows).  start (device): q_syrk rows of Npad doubles -- the data's alpha (q_syrk = q = 1), REML's [alpha_R; C], or zeros
// (with trend rows in front of the unit rows the rank-q kernel, q_syrk = 2: it reads `dense`).  The launch lies between ev0
// and ev1: lik_ginv_ms behind the caller's next synchronisation.
static int lik_ginv(ck_handle* h, const double* start, int q_syrk, int q) {
    if (schur_ensure(h, h->Npad)) return -1;
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    ck_launch_ginv_syrk(h->stream, h->sch.d_ptr, h->aux, h->mpad, start, h->nK, h->nend, q_syrk, h->Npad, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    return 0;
}
static double lik_ginv_ms(const ck_handle* h) { return elapsed_ms(h->ev0, h->ev1); }

// The five-point stencil in nu of the model's blocks -- 3 blocks x (the block, nu - 2 d, nu - d, nu + d, nu + 2 d), d = dnu3[b]
// -- built in the handle's staging array and queued for d_lik_blk.  One process: its block in all three places.
static int lik_blocks(ck_handle* h, double dnu3[3]) {
    const int nblk = h->n_procs == 1 ? 1 : 3;
    const double offs[4] = {-2.0, -1.0, 1.0, 2.0};
    CkMatern* hb = h->lik_hb;
    for (int b = 0; b < 3; ++b) {
        const CkMatern& m = h->blk[b < nblk ? b : 0];
        dnu3[b] = ck_matern_dnu_step(m.nu);
        hb[5 * b] = m;
        for (int k = 0; k < 4; ++k) ck_matern_prepare(m.nu + offs[k] * dnu3[b], m.len_scale, m.amp, m.nugget, &hb[5 * b + 1 + k]);
    }
    HIPCHK(h->d_lik_blk.reserve(sizeof(h->lik_hb) / sizeof(CkMatern)));
    HIPCHK(hipMemcpyAsync(h->d_lik_blk, hb, sizeof(h->lik_hb), hipMemcpyHostToDevice, h->stream));
    return 0;
}

// The live parameter slots of a 13-slot score or information (bit k): the model's parameters, the noise scale of a process
// that has variances, less what free13 (may be null) fixes.
static unsigned live_slots(const ck_handle* h, const int32_t* free13) {
    unsigned live = 0;
    const int npar = h->n_procs == 1 ? 4 : CK_LIK_NPAR;
    for (int k = 0; k < npar; ++k) live |= 1u << k;
    if (!h->noise_var[0].empty()) live |= 1u << 11;
    if (h->n_procs == 2 && !h->noise_var[1].empty()) live |= 1u << 12;
    if (free13)
        for (int k = 0; k < CK_FISHER_NPAR; ++k)
            if (free13[k] == 0) live &= ~(1u << k);
    return live;
}

// grad[0 .. npar) <- the contraction of G (in the Schur buffers, behind lik_ginv) with the derivatives of Sigma; *ms: its
// device window (ev1 .. ev2).  Synchronises the stream.
static int lik_contract(ck_handle* h, DevTemps& tmp, int npar, double* grad, double* ms) {
    const CkLayout L = layout_of(h);
    double dnu3[3] = {0.0, 0.0, 0.0};
    if (lik_blocks(h, dnu3)) return -1;
    const int64_t ngr = ck_lik_grad_groups(L);
    double* d_part = nullptr;
    HIPCHK(tmp.get(&d_part, (size_t)(ngr * CK_LIK_NPAR) * 8));
    ck_launch_loglik_grad(h->stream, h->sch.d_ptr, L, h->n_procs, h->metric, h->s0, h->d_lik_blk, dnu3, h->par_sigma[0],
                          h->par_sigma[1], h->par_rho, d_part);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev2, h->stream));
    std::vector<double> part((size_t)(ngr * CK_LIK_NPAR));
    HIPCHK(hipMemcpyAsync(part.data(), d_part, part.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *ms = elapsed_ms(h->ev1, h->ev2);
    double g[CK_LIK_NPAR] = {};
    for (int64_t w = 0; w < ngr; ++w)
        for (int k = 0; k < CK_LIK_NPAR; ++k) g[k] += part[(size_t)(w * CK_LIK_NPAR + k)];
    for (int k = 0; k < npar; ++k) grad[k] = g[k];
    return 0;
}

// dl/ds_k = 1/2 sum_{a in k} G_aa d_a while G is in the Schur buffers: what ck_loglik_noise_grad hands out
static int lik_noise_scores(ck_handle* h, DevTemps& tmp) {
    h->lik_noise_grad[0] = h->lik_noise_grad[1] = 0.0;
    if (ensure_noise(h)) return -1;
    if (!h->noise_var[0].empty() || (h->n_procs == 2 && !h->noise_var[1].empty())) {
        double* d_np = nullptr;
        HIPCHK(tmp.get(&d_np, (size_t)(2 * h->nK) * 8));
        ck_launch_lik_noise_grad(h->stream, h->sch.d_ptr, h->nK, layout_of(h), h->d_noise + h->Npad, d_np);
        HIPCHK(hipGetLastError());
        std::vector<double> np2((size_t)(2 * h->nK));
        HIPCHK(hipMemcpyAsync(np2.data(), d_np, np2.size() * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        for (int K = 0; K < h->nK; ++K)
            for (int k = 0; k < 2; ++k) h->lik_noise_grad[k] += np2[(size_t)(2 * K + k)];
        for (int k = 0; k < 2; ++k) h->lik_noise_grad[k] *= 0.5;
    }
    h->lik_noise_valid = true;
    return 0;
}

// ck_loglik (p = 0, three outputs) and ck_loglik_reml (p = the trend columns, four)
static int loglik_value_grad(ck_handle* h, const char* name, bool reml, int want_grad, double* out, double* grad, int64_t* info) {
    if (lik_admit(h, name, !out || !info || (want_grad && !grad))) return -1;
    const auto t_begin = std::chrono::steady_clock::now();
    const int64_t Np = h->Npad;
    const int npar = h->n_procs == 1 ? 4 : CK_LIK_NPAR;
    const int p = reml ? trend_total(h) : 0;   // trend columns (0: the zero-mean likelihood)
    const int q = 1 + p;
    *info = 0;
    for (int k = 0; k < (reml ? 4 : 3); ++k) out[k] = NAN;
    if (want_grad) {
        for (int k = 0; k < npar; ++k) grad[k] = NAN;
        CkMemAdmit a;
        if (lik_mem_admit(h, name, p, &a)) return -1;
        if (a.need > a.avail) {
            const int64_t aux_bytes = rhs_bytes(roundup(Np + 1 + p, CK_AUX_ALIGN), Np);
            return fail(std::string(name) + ": the gradient needs " + std::to_string(aux_bytes + schur_bytes(Np)) +
                        " bytes of device memory (" + std::to_string(aux_bytes) + " for " + std::to_string(Np + 1 + p) + " rows of " +
                        std::to_string(Np) + " doubles, " + std::to_string(schur_bytes(Np)) + " for the lower triangle of G); " +
                        std::to_string(a.avail) + " bytes are available");
        }
    }
    CallGuard guard(h, AUX_LOGLIK, true);
    double* t = h->t_ms;
    timings_from(h, 24);
    DevTemps tmp;
    LikSweep S;
    const int rc = lik_sweep(h, tmp, name, want_grad != 0, p, false, &S);
    *info = S.info;
    if (rc) return -1;
    t[24] = t[0];   // the assembly of this Sigma (ck_assemble_joint)
    if (S.factored_here) t[25] = t[1];
    if (S.info != 0) {
        t[29] = ms_since(t_begin);
        return 0;
    }
    t[26] = S.sweep_ms;
    out[1] = S.logdet;
    if (reml) {
        out[2] = S.logdetA;
        out[3] = S.quad;
        out[0] = -0.5 * ((double)(h->N - p) * log(2.0 * M_PI) + S.logdet + S.logdetA + S.quad);
    } else {
        out[2] = S.quad;
        out[0] = -0.5 * ((double)h->N * log(2.0 * M_PI) + S.logdet + S.quad);
    }
    if (want_grad) {
        // ---- G = alpha alpha^T - Sigma^-1 (REML: alpha_R alpha_R^T + C C^T - Sigma^-1), its contraction and the noise scores
        const double* start = h->d_pred + 1;
        std::vector<double> av;
        if (p > 0) {
            av.assign((size_t)q * Np, 0.0);
            ck_host_reml_start(p, Np, S.W.data(), q, S.beta.data(), S.R.data(), av.data());
            double* d_av = nullptr;
            HIPCHK(tmp.get(&d_av, av.size() * 8));
            HIPCHK(hipMemcpyAsync(d_av, av.data(), av.size() * 8, hipMemcpyHostToDevice, h->stream));
            start = d_av;
        }
        if (lik_ginv(h, start, q, q)) return -1;
        if (lik_contract(h, tmp, npar, grad, &t[28])) return -1;
        t[27] = lik_ginv_ms(h);
        if (lik_noise_scores(h, tmp)) return -1;
    }
    t[29] = ms_since(t_begin);
    return 0;
}

extern "C" int ck_loglik(ck_handle* h, int want_grad, double* out3, double* grad, int64_t* info) {
    CHKH(h);
    return loglik_value_grad(h, "ck_loglik", false, want_grad, out3, grad, info);
}

extern "C" int ck_loglik_reml(ck_handle* h, int want_grad, double* out4, double* grad, int64_t* info) {
    CHKH(h);
    return loglik_value_grad(h, "ck_loglik_reml", true, want_grad, out4, grad, info);
}

extern "C" int ck_loglik_noise_grad(ck_handle* h, double* out2) {
    CHKH(h);
    if (!out2) return fail("ck_loglik_noise_grad: null argument");
    if (!h->lik_noise_valid)
        return fail("ck_loglik_noise_grad: no ck_loglik / ck_loglik_reml with want_grad != 0 has succeeded on this handle since the "
                    "last ck_assemble_joint");
    out2[0] = h->lik_noise_grad[0];
    out2[1] = h->lik_noise_grad[1];
    return 0;
}

// ---------------------------------------------------------------------------------------
// Fisher information of the likelihood fit (ck_fisher.hip)
// ---------------------------------------------------------------------------------------
// I_jk = 1/2 tr(Sigma^-1 D_j Sigma^-1 D_k) in the plain form.  lik_sweep and lik_ginv leave -Sigma^-1 in the Schur buffers (zero
// start); it is expanded to full K-panels, the derivative operands (ck_internal.h: CK_FOP_*) are assembled as the product
// kernel's second operand, B_a = -Sigma^-1 D_a runs on the trailing updates' tile restricted to the operand's block (N^3 / 2
// flop for an operand inside one process of a half-and-half model, N^3 for a cross operand), and one contraction kernel takes
// all wanted pairs to per-workgroup partial sums.  The products of all operands are kept when they fit; otherwise the operands
// are cut into groups of at most half the free memory, and the pairs across two groups are contracted with the later group's
// products formed again (memory first: the need is computed in front of the first allocation).
static_assert(CK_HOST_FOP_R11 == CK_FOP_R11 && CK_HOST_FOP_R01 == CK_FOP_R01 && CK_HOST_FOP_DIAG0 == CK_FOP_DIAG0 &&
                  CK_HOST_FISHER_YROWS == CK_FISHER_YROWS && CK_HOST_FISHER_NOPS == CK_FISHER_NOPS,
              "ck_host.h and ck_internal.h disagree about the Fisher operands");
extern "C" int ck_loglik_fisher(ck_handle* h, int reml, const int32_t* free13, double* fisher, int64_t* info) {
    CHKH(h);
    const char* name = "ck_loglik_fisher";
    if (lik_admit(h, name, !fisher || !info)) return -1;
    const auto t_begin = std::chrono::steady_clock::now();
    const int NP = CK_FISHER_NPAR, NO = CK_FISHER_NOPS;
    *info = 0;
    for (int k = 0; k < NP * NP; ++k) fisher[k] = NAN;
    const int64_t Np = h->Npad;
    const int nK = h->nK;
    const int p = reml ? trend_total(h) : 0;
    // ---- live slots and the operands they need
    unsigned char live[CK_FISHER_NPAR] = {};
    const unsigned live_mask = live_slots(h, free13);
    for (int k = 0; k < NP; ++k) live[k] = live_mask >> k & 1u;
    double coef[CK_FISHER_NPAR * CK_FISHER_NOPS];
    ck_host_fisher_coef(h->n_procs, h->par_sigma[0], h->par_sigma[1], h->par_rho, coef);
    bool op_live[CK_FISHER_NOPS] = {};
    for (int k = 0; k < NP; ++k)
        for (int a = 0; a < NO; ++a)
            if (live[k] && coef[k * NO + a] != 0.0) op_live[a] = true;
    // ---- memory, in front of the first allocation: the unit-row sweep and G as ck_loglik's gradient takes them; Sigma^-1, the
    // operands, the thin REML terms and the partial sums whole; the products in as many groups as fit (ck_host_fisher_plan)
    CkMemAdmit adm;
    if (lik_mem_admit(h, name, p, &adm)) return -1;
    CkFisherPlan P;
    if (ck_host_fisher_plan(h->n_procs, Np, h->n0p, nK, op_live, adm.avail - adm.need, p, ck_fisher_contract_groups(Np),
                            h->fisher_product_mb << 20, &P))
        return fail(std::string(name) + ": needs " + std::to_string(adm.need + P.fixed_bytes + 2 * P.b_max * 8) +
                    " bytes of device memory (" + std::to_string(adm.need) + " for the unit-row sweep and Sigma^-1's triangle, " +
                    std::to_string(Np * Np * 8) + " for Sigma^-1 in full, " + std::to_string(P.d_total * 8) + " for " +
                    std::to_string(P.units.size()) + " derivative operands, " + std::to_string(2 * P.b_max * 8) +
                    " for two of their products); " + std::to_string(adm.avail) + " bytes are available");
    const std::vector<CkFisherUnit0>& units = P.units;
    const std::vector<std::vector<int>>& groups = P.groups;
    const int64_t *c0 = P.c0, *wpad = P.wpad, *nlo = P.nlo, *nhi = P.nhi, *b_doubles = P.b_doubles, region = P.region;
    const int *pK0 = P.pK0, *npan = P.npan;
    const int64_t ngr = ck_fisher_contract_groups(Np);
    // ---- the sweep: factor, unit rows, -Sigma^-1 in the Schur buffers (and A, H of REML)
    CallGuard guard(h, AUX_LOGLIK, true);
    double* t = h->t_ms;
    timings_from(h, 24);
    DevTemps tmp;
    LikSweep S;
    {
        const int rc = lik_sweep(h, tmp, name, true, p, true, &S);
        *info = S.info;
        if (rc) return -1;
    }
    t[24] = t[0];
    if (S.factored_here) t[25] = t[1];
    if (S.info != 0) {
        t[29] = t[67] = ms_since(t_begin);
        return 0;
    }
    t[26] = S.sweep_ms;
    {
        const int q_syrk = p > 0 ? 2 : 1;
        double* d_zero = nullptr;
        HIPCHK(tmp.get(&d_zero, (size_t)(q_syrk * Np) * 8));
        HIPCHK(hipMemsetAsync(d_zero, 0, (size_t)(q_syrk * Np) * 8, h->stream));
        if (lik_ginv(h, d_zero, q_syrk, 1 + p)) return -1;
        HIPCHK(hipStreamSynchronize(h->stream));
        t[27] = lik_ginv_ms(h);
        t[29] = ms_since(t_begin);
    }
    const CkLayout L = layout_of(h);
    if (ensure_noise(h)) return -1;
    double *d_Sp = nullptr, *d_part = nullptr, *d_reg[2] = {nullptr, nullptr};
    HIPCHK(tmp.get(&d_Sp, (size_t)(Np * Np) * 8));
    HIPCHK(tmp.get(&d_part, (size_t)(ngr * CK_FISHER_NPAIR) * 8));
    std::vector<double*> d_D(units.size(), nullptr);
    for (size_t u = 0; u < units.size(); ++u) {
        HIPCHK(tmp.get(&d_D[u], (size_t)units[u].d_doubles * 8));
        HIPCHK(hipMemsetAsync(d_D[u], 0, (size_t)units[u].d_doubles * 8, h->stream));
    }
    if (region > 0) HIPCHK(tmp.get(&d_reg[0], (size_t)region * 8));
    if (groups.size() > 1) HIPCHK(tmp.get(&d_reg[1], (size_t)region * 8));
    // ---- Sigma^-1 in full; the operands
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    ck_launch_fisher_expand(h->stream, h->sch.d_ptr, L, d_Sp);
    HIPCHK(hipGetLastError());
    CkFisherAsm A = {};
    for (int r = 0; r < 2; ++r) A.c0[r] = c0[r], A.wpad[r] = wpad[r], A.pK0[r] = pK0[r];
    for (size_t u = 0; u < units.size(); ++u) A.D[units[u].op][units[u].r] = d_D[u];
    if (!units.empty()) {
        double dnu3[3] = {0.0, 0.0, 0.0};
        if (lik_blocks(h, dnu3)) return -1;
        ck_launch_fisher_assemble(h->stream, A, L, h->n_procs, h->metric, h->s0, h->d_lik_blk, dnu3);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    t[64] = elapsed_ms(h->ev0, h->ev1);
    // ---- products and contraction, group by group
    const CkFisherCtx X{d_Sp, h->d_noise ? h->d_noise + Np : nullptr, Np, h->n_procs == 2 ? h->n0p : Np, h->n_procs};
    double T[CK_FISHER_NOPS * CK_FISHER_NOPS] = {};
    double flop = 0.0;
    CkFisherOp desc[CK_FISHER_NOPS] = {};
    for (int k = 0; k < 2; ++k)
        if (op_live[CK_FOP_DIAG0 + k]) desc[CK_FOP_DIAG0 + k] = CkFisherOp{nullptr, 0, 0, 0, CK_FOPK_DIAG0 + k};
    auto form = [&](const std::vector<int>& g, double* reg) -> int {   // the products of a group into a region
        int64_t off = 0;
        for (int a : g) {
            double* B = reg + off;
            off += b_doubles[a];
            HIPCHK(hipMemsetAsync(B, 0, (size_t)b_doubles[a] * 8, h->stream));
            const bool cross = a >= CK_FOP_R01;
            const int r0 = a < CK_FOP_R11 ? 0 : 1;
            desc[a] = cross ? CkFisherOp{B, Np, 0, Np, CK_FOPK_DENSE} : CkFisherOp{B, wpad[r0], c0[r0], wpad[r0], CK_FOPK_DENSE};
            for (size_t u = 0; u < units.size(); ++u) {
                if (units[u].op != a) continue;
                const int r = units[u].r, kp = units[u].kp;
                ck_launch_fisher_prod(h->stream, cross ? B + c0[r] : B, cross ? Np : wpad[r], d_Sp, Np, d_D[u], wpad[r], pK0[kp],
                                      npan[kp]);
                flop += 2.0 * (double)Np * (double)wpad[r] * (double)npan[kp] * CK_NB;
            }
        }
        HIPCHK(hipGetLastError());
        return 0;
    };
    std::vector<double> part((size_t)(ngr * CK_FISHER_NPAIR));
    auto group_of = [&](int a) -> int {
        for (size_t g = 0; g < groups.size(); ++g)
            for (int x : groups[g])
                if (x == a) return (int)g;
        return 0;   // the diagonal operands ride with the first group
    };
    auto contract = [&](int ga, int gb) -> int {   // the pairs with one operand in group ga and the other in gb
        CkFisherOps O = {};
        bool any = false;
        for (int a = 0; a < NO; ++a) {
            O.op[a] = desc[a];
            if (!op_live[a]) continue;
            for (int b = a; b < NO; ++b) {
                if (!op_live[b]) continue;
                const int x = group_of(a), y = group_of(b);
                if ((x == ga && y == gb) || (x == gb && y == ga)) O.mask[a] |= 1u << b, any = true;
            }
        }
        if (!any) return 0;
        ck_launch_fisher_contract(h->stream, O, X, d_part);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(part.data(), d_part, part.size() * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        for (int a = 0; a < NO; ++a)
            for (int b = a; b < NO; ++b) {
                if (!((O.mask[a] >> b) & 1u)) continue;
                double s = 0.0;
                for (int64_t w = 0; w < ngr; ++w) s += part[(size_t)(w * CK_FISHER_NPAIR + b * (b + 1) / 2 + a)];
                T[a * NO + b] = T[b * NO + a] = 0.5 * s;
            }
        return 0;
    };
    auto timed = [&](int slot, auto fn) -> int {
        HIPCHK(hipEventRecord(h->ev0, h->stream));
        if (fn()) return -1;
        HIPCHK(hipEventRecord(h->ev1, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        h->t_ms[slot] += elapsed_ms(h->ev0, h->ev1);
        return 0;
    };
    for (int ga = 0; ga < (int)groups.size(); ++ga) {
        if (timed(65, [&]() { return form(groups[(size_t)ga], d_reg[0]); })) return -1;
        if (timed(66, [&]() { return contract(ga, ga); })) return -1;
        for (int gb = ga + 1; gb < (int)groups.size(); ++gb) {
            if (timed(65, [&]() { return form(groups[(size_t)gb], d_reg[1]); })) return -1;
            if (timed(66, [&]() { return contract(ga, gb); })) return -1;
        }
    }
    // ---- REML: the thin terms Y_a = D_a H, V = Sigma^-1 Y, K = Y^T V, Gm = Y^T H and the p x p algebra on the host
    if (p > 0) {
        double *d_H = nullptr, *d_Yp = nullptr, *d_V = nullptr, *d_K = nullptr;
        const int64_t yp_doubles = (int64_t)nK * CK_FISHER_YROWS * CK_NB;
        HIPCHK(tmp.get(&d_H, (size_t)(Np * p) * 8));
        HIPCHK(tmp.get(&d_Yp, (size_t)yp_doubles * 8));
        HIPCHK(tmp.get(&d_V, (size_t)(Np * CK_FISHER_YROWS) * 8));
        HIPCHK(tmp.get(&d_K, (size_t)(CK_FISHER_YROWS * (CK_FISHER_YROWS + p)) * 8));
        HIPCHK(hipEventRecord(h->ev0, h->stream));
        HIPCHK(hipMemcpyAsync(d_H, S.H.data(), (size_t)(Np * p) * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemsetAsync(d_Yp, 0, (size_t)yp_doubles * 8, h->stream));
        HIPCHK(hipMemsetAsync(d_V, 0, (size_t)(Np * CK_FISHER_YROWS) * 8, h->stream));
        for (size_t u = 0; u < units.size(); ++u) {
            const int r = units[u].r, kp = units[u].kp;
            const CkFisherUnit U{d_D[u], c0[r], wpad[r], nlo[r], nhi[r], pK0[kp], npan[kp]};
            ck_launch_fisher_dh(h->stream, U, d_H, p, units[u].op * p, d_Yp);
        }
        for (int k = 0; k < 2; ++k)
            if (op_live[CK_FOP_DIAG0 + k])
                ck_launch_fisher_dh_diag(h->stream, L, h->n_procs, k, X.d, d_H, p, (CK_FOP_DIAG0 + k) * p, d_Yp);
        ck_launch_fisher_prod(h->stream, d_V, CK_FISHER_YROWS, d_Sp, Np, d_Yp, CK_FISHER_YROWS, 0, nK);
        flop += 2.0 * (double)Np * CK_FISHER_YROWS * (double)Np;
        ck_launch_fisher_ytv(h->stream, d_Yp, Np, d_V, CK_FISHER_YROWS, CK_FISHER_YROWS, d_K, CK_FISHER_YROWS);
        double* d_Gm = d_K + CK_FISHER_YROWS * CK_FISHER_YROWS;
        ck_launch_fisher_ytv(h->stream, d_Yp, Np, d_H, p, p, d_Gm, p);
        HIPCHK(hipGetLastError());
        std::vector<double> Kh((size_t)(CK_FISHER_YROWS * (CK_FISHER_YROWS + p)));
        HIPCHK(hipMemcpyAsync(Kh.data(), d_K, Kh.size() * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipEventRecord(h->ev1, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        h->t_ms[65] += elapsed_ms(h->ev0, h->ev1);
        for (size_t k = 0; k < (size_t)(CK_FISHER_YROWS * CK_FISHER_YROWS); ++k) Kh[k] = -Kh[k];   // V holds -Sigma^-1 Y
        if (ck_host_fisher_reml(p, NO, S.A.data(), Kh.data(), CK_FISHER_YROWS, Kh.data() + CK_FISHER_YROWS * CK_FISHER_YROWS, T))
            return fail(std::string(name) + ": X^T Sigma^-1 X did not factor");
    }
    ck_host_fisher_combine(coef, T, live, fisher);
    h->t_ms[68] = flop;
    h->t_ms[69] = (double)groups.size();
    h->t_ms[67] = ms_since(t_begin);
    return 0;
}

// ---------------------------------------------------------------------------------------
// local-neighbourhood cokriging: src/point_prediction.py:45-249
// ---------------------------------------------------------------------------------------
// largest chord (in the space of su / pu) a neighbour can have, with a margin (ck_local.hip: lp_chunk_far)
static double local_cmax(const ck_handle* h, double max_dist) {
    double cmax = max_dist;
    if (h->metric == CK_METRIC_HAVERSINE) {
        const double half = max_dist / (2.0 * CK_EARTH_RADIUS_KM);
        cmax = half >= 1.5 ? 4.0 : 2.0 * sin(half);   // beyond ~ a quarter of the globe: no culling
    }
    cmax = cmax * (1.0 + 1e-9) + 1e-12;
    return cmax == cmax ? cmax : INFINITY;
}
// What the handle knows of a local call (ck_internal.h: CkLocalProblem); the caller adds its points and the search's cap /
// precedence pointers.  Behind ensure_layout and ensure_noise.
static CkLocalProblem local_problem(const ck_handle* h, int i, int cv, double max_dist) {
    CkLocalProblem P;
    P.blk = h->d_blk;
    P.tabs = h->d_tabs;
    P.coefs = h->d_coefptr;
    P.use_tab = tables_usable(h) ? 1 : 0;
    P.metric = h->metric;
    P.i_pred = i;
    P.cv = cv ? 1 : 0;
    if (cv) P.lo[i] = 0.0;   // the co-located data of process i
    P.max_dist = max_dist;
    P.c0var = h->blk[2 * i].amp + h->blk[2 * i].nugget;   // covariance(i, 0)[0], point_prediction.py:66
    P.sc = h->s0;
    P.su = h->su;
    P.z = h->z;
    P.L = layout_of(h);
    P.nz = noise_sd(h);   // measurement-error variances on the diagonal of every local system (null: off)
    P.cb = h->d_chunkb;
    P.cmax = local_cmax(h, max_dist);
    return P;
}

// the neighbour cap of process q as the kernels take it (a cap beyond INT_MAX binds nowhere; one process: no second cap)
static int local_nmax_of(const ck_handle* h, int q) {
    if (q >= h->n_procs) return 0;
    return (int)std::min<int64_t>(h->local_nmax[q], INT32_MAX);
}
static int local_key_cap(const ck_handle* h) {
    return h->local_select_cap > 0 ? h->local_select_cap : ck_local_select_capacity();
}
// What the select pass reports (all zero: an uncapped call, whose counting pass is no select pass); ck_timings [60 .. 63]
struct LocalSelectStats {
    double ms = 0.0;                                    // the pass's device window
    int64_t n_capped = 0, cand_max = 0, n_rescan = 0;   // points with a capped process | largest candidate count (both
                                                        // processes) before the cap | points that re-scanned
    void add(const LocalSelectStats& o) {               // over several passes (the Vecchia entry points: one per process)
        ms += o.ms;
        n_capped += o.n_capped;
        cand_max = std::max(cand_max, o.cand_max);
        n_rescan += o.n_rescan;
    }
};
static void write_select_timings(ck_handle* h, const LocalSelectStats& st) {
    h->t_ms[60] = st.ms;
    h->t_ms[61] = (double)st.n_capped;
    h->t_ms[62] = (double)st.cand_max;
    h->t_ms[63] = (double)st.n_rescan;
}

// The first stage of every local call: the points on the device and their counting or select pass.  What it leaves behind is
// what the later launches of the call are told (prob) and what the host plans with (cnt; sel: m x 4 ints of a select pass).
struct LocalPass {
    int64_t m = 0, mp = 0;
    double *d_p3 = nullptr, *d_pu = nullptr, *d_rq = nullptr, *d_cp = nullptr;   // d_rq, d_cp: select pass only
    int *d_cnt = nullptr, *d_sel = nullptr, *d_rp = nullptr;                     // d_sel: select pass only; d_rp: with rp_host
    int* d_fp = nullptr;                                                         // with the fold labels of a withholding call
    CkLocalProblem prob;
    std::vector<int> cnt, sel;
    double pass_ms = 0.0;   // the pass's device window, whichever pass it was
    LocalSelectStats st;
};
// select: the select pass with the handle's caps (the counting pass of a capped call); else the counting pass, and no kernel
// sees a cap pointer.  d_rs / rp_host: the precedence condition of the Vecchia likelihood (device: every site's position in the
// ordering; host: the m points'), both null without one.  rcut_host: m x 2, receives the cut distances of a select pass.  One
// synchronisation, after the downloads; pass_ms is read here, so [ev0, ev1] are free again when the stage returns.
// wh: the withholding conditions of ck_cv_local_folds (null: none, and no kernel sees a label or a radius).
struct LocalWithhold {
    const int* d_fs;   // device: every site's fold label in the internal site order (Npad ints), or null: no fold condition
    const int* fp;     // host: the m points' labels (read with d_fs)
    double wb[2];      // the buffer radius of process 0 / 1, negative: off
};
static int local_pass(ck_handle* h, DevTemps& tmp, int i, const double* pcoords, int64_t m, double max_dist, int cv, bool select,
                      const int* d_rs, const int* rp_host, double* rcut_host, LocalPass* out, const LocalWithhold* wh = nullptr) {
    LocalPass& S = *out;
    const int64_t mp = S.mp = roundup(S.m = m, 64);
    double* d_pc = nullptr;
    HIPCHK(tmp.get(&d_pc, (size_t)(2 * mp * 8)));
    HIPCHK(tmp.get(&S.d_p3, (size_t)(3 * mp * 8)));
    HIPCHK(tmp.get(&S.d_pu, (size_t)(3 * mp * 8)));
    HIPCHK(tmp.get(&S.d_cnt, (size_t)(mp * sizeof(int))));
    if (select) {
        HIPCHK(tmp.get(&S.d_sel, (size_t)(4 * mp * sizeof(int))));
        HIPCHK(tmp.get(&S.d_rq, (size_t)(2 * mp * 8)));
        HIPCHK(tmp.get(&S.d_cp, (size_t)(mp * 8)));
    }
    if (rp_host) {
        HIPCHK(tmp.get(&S.d_rp, (size_t)(mp * sizeof(int))));
        HIPCHK(hipMemcpyAsync(S.d_rp, rp_host, (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
    }
    if (wh && wh->d_fs) {
        HIPCHK(tmp.get(&S.d_fp, (size_t)(mp * sizeof(int))));
        HIPCHK(hipMemcpyAsync(S.d_fp, wh->fp, (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(hipMemsetAsync(d_pc, 0, 2 * mp * 8, h->stream));
    HIPCHK(hipMemcpyAsync(d_pc, pcoords, 2 * m * 8, hipMemcpyHostToDevice, h->stream));
    ck_launch_prep_sites(h->stream, d_pc, mp, h->metric, S.d_p3, S.d_p3 + mp, S.d_p3 + 2 * mp, S.d_pu);
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    S.prob = local_problem(h, i, cv, max_dist);
    if (wh) {
        S.prob.fs = wh->d_fs;
        S.prob.fp = S.d_fp;
        for (int q = 0; q < 2; ++q)
            if (wh->wb[q] >= 0.0) {
                S.prob.cv = 1;
                S.prob.lo[q] = std::max(S.prob.lo[q], wh->wb[q]);
            }
    }
    S.prob.pc = S.d_p3;
    S.prob.pu = S.d_pu;
    S.prob.mpad = mp;
    S.prob.rq = S.d_rq;
    S.prob.cp = S.d_cp;
    S.prob.rs = d_rs;
    S.prob.rp = S.d_rp;
    S.prob.listed = (d_rs || S.prob.fs) ? 1 : 0;
    if (select)
        ck_launch_local_select(h->stream, S.prob, m, local_nmax_of(h, 0), local_nmax_of(h, 1), local_key_cap(h), S.d_cnt, S.d_sel,
                               S.d_rq, S.d_cp);
    else
        ck_launch_local_count(h->stream, S.prob, m, S.d_cnt);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    S.cnt.resize((size_t)m);
    if (select) {   // the counts are the sum of its first two columns (ck_internal.h): one download
        S.sel.resize((size_t)(4 * m));
        HIPCHK(hipMemcpyAsync(S.sel.data(), S.d_sel, S.sel.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        if (rcut_host) HIPCHK(hipMemcpyAsync(rcut_host, S.d_rq, (size_t)(2 * m * 8), hipMemcpyDeviceToHost, h->stream));
    } else {
        HIPCHK(hipMemcpyAsync(S.cnt.data(), S.d_cnt, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(elapsed_ms(h->ev0, h->ev1, &S.pass_ms));
    if (select) {
        S.st.ms = S.pass_ms;
        for (int64_t p = 0; p < m; ++p) {
            const int* s = &S.sel[(size_t)(4 * p)];
            S.cnt[(size_t)p] = s[0] + s[1];
            S.st.n_capped += (s[3] & CK_LS_CAPPED) != 0;
            S.st.n_rescan += (s[3] & CK_LS_RESCAN) != 0;
            S.st.cand_max = std::max<int64_t>(S.st.cand_max, s[2]);
        }
    }
    return 0;
}

// The slab budget of the large-neighbourhood paths in doubles: a quarter of the free device memory, the kept slab counted as
// free (it is ours to reuse), at most 32 GiB; option "local_slab_mb" if set (tests).  *avail: the bytes that count as free.
static int local_budget_doubles(const ck_handle* h, long long* budget, size_t* avail = nullptr) {
    size_t mem_free = 0, mem_total = 0;
    HIPCHK(hipMemGetInfo(&mem_free, &mem_total));
    mem_free += (size_t)local_slab_doubles(h) * 8;
    *budget = (long long)std::min<size_t>(mem_free / 4, (size_t)32 << 30) / 8;
    if (h->local_slab_mb > 0) *budget = (long long)h->local_slab_mb * (1 << 20) / 8;
    if (avail) *avail = mem_free;
    return 0;
}
// The kept slab grown to at least `need` doubles (no-op when it is that large); *grow_ms: what that cost (ck_timings [14]).
// Growing is what stalls: hipMalloc of tens of GiB right after a hipFree of a few GiB that were written took 1-4 s every time
// (scripts/diag_malloc.py; profiles/r03c_local_predictor.json's 100 km row, 1 262 ms for a 3 ms call, was this allocation).
// So: beyond 1 GiB take the whole budget at once (the slab then never grows again), and allocate the new slab before
// releasing the old one; without room for both, release first and take what is needed.
static int local_slab_grow(ck_handle* h, long long need, long long budget, double* grow_ms) {
    *grow_ms = 0.0;
    if (need <= local_slab_doubles(h)) return 0;
    const auto t_grow = std::chrono::steady_clock::now();
    const long long want = need * 8 > (1LL << 30) ? std::max(need, budget) : need;
    DevBuf<double> fresh;
    if (fresh.reserve((size_t)want) != hipSuccess) {
        (void)hipGetLastError();
        h->local_slab.reset();
        HIPCHK(fresh.reserve((size_t)need));
    }
    h->local_slab = std::move(fresh);   // releases the old slab
    *grow_ms = ms_since(t_grow);
    return 0;
}

extern "C" int ck_set_local_neighbours(ck_handle* h, int64_t nmax0, int64_t nmax1) {
    CHKH(h);
    if (nmax0 < 0 || nmax1 < 0)
        return fail("ck_set_local_neighbours: a cap must be >= 0 (0 = none), got (" + std::to_string(nmax0) + ", " +
                    std::to_string(nmax1) + ")");
    h->local_nmax[0] = nmax0;
    h->local_nmax[1] = nmax1;
    return 0;
}

// the select pass alone, with the handle's caps (none: the candidate counts and max_dist)
extern "C" int ck_debug_local_neighbours(ck_handle* h, int i, const double* pcoords, int64_t m, double max_dist, int cv,
                                         int32_t* count, double* rcut) {
    CHKH(h);
    if (ensure_layout(h, false)) return -1;
    if (i < 0 || i >= h->n_procs) return fail("process index out of range");
    if (m < 0 || (m > 0 && (!pcoords || !count || !rcut))) return fail("ck_debug_local_neighbours: bad arguments");
    timings_from(h, 60);
    DevTemps tmp;
    LocalPass S;   // (the select pass reads neither the values nor the noise)
    if (m > 0 && local_pass(h, tmp, i, pcoords, m, max_dist, cv, true, nullptr, nullptr, rcut, &S)) return -1;
    for (int64_t p = 0; p < m; ++p) {
        count[2 * p] = S.sel[(size_t)(4 * p)];
        count[2 * p + 1] = S.sel[(size_t)(4 * p + 1)];
    }
    write_select_timings(h, S.st);
    return 0;
}

// The universal form's extras (ck_predict_local_universal); null: simple cokriging, ck_predict_local as it always was
struct LocalUniv {
    const double* f0;      // m x p_i, the caller's (may hold non-finite entries: rule 5)
    double* beta;          // m x p or null
    int64_t* n_rank_def;
};

// The Vecchia likelihood's extras (ck_loglik_vecchia); null: a prediction.  The points are the data of process i in the caller's
// order; a site is a neighbour only if it comes earlier in the ordering than the point.  The select pass always runs (it is
// what counts per process), with the handle's caps or none.
struct LocalVecchia {
    const int* d_rs;      // device: position in the ordering of every site, internal site order (Npad ints)
    const int* rp;        // host: the m points' positions
    double* vv;           // host, m: the raw v . v of every solved point (0 where the set is empty)
    int32_t* cnt2;        // host, m x 2: conditioning data of process 0 / 1
};

// Block cokriging's extras (ck_predict_local_blocks); null: a point call.  The points of the call are the blocks' search
// centres; the members (lay: ck_host_local_block_layout) enter the c row and the prior variance only.
struct LocalBlocks {
    const CkLocalBlockLayout* lay;
};

// What a call of predict_local_impl reports: to the caller, and to ck_timings through the exported entry points
struct LocalResult {
    int64_t n_empty = 0, n_not_pd = 0, k_max = 0;
    int64_t n_tiled = 0;        // points of the tiled class
    int64_t n_tbatches = 0;     // batches the tiled class was cut into under the slab budget
    double pass_ms = 0.0;       // device windows: the counting pass (a capped call's select pass),
    double solve_ms = 0.0;      // assembly / factorisations / reductions,
    double reduce_ms = 0.0;     // of which the tiled class's universal reductions (universal form)
    double grow_ms = 0.0;       // host: a growth of the scratch slab, between the two device windows
    double total_ms = 0.0;      // host: the call (universal form, block form)
    double lds_ms = 0.0;        // block form: the LDS class's launch inside solve_ms,
    double prior_ms = 0.0;      // the sigma_BB pass (its own device window, in front of the solve window),
    double cbar_evals = 0.0;    // sum_b q_b k_b: the member-neighbour covariance evaluations
    LocalSelectStats st;
};
// ck_timings [10] device work, [14] slab growth, [60 .. 63] the select pass (zeros after an uncapped call)
static void write_local_timings(ck_handle* h, const LocalResult& R) {
    h->t_ms[10] = R.pass_ms + R.solve_ms;
    h->t_ms[14] = R.grow_ms;
    write_select_timings(h, R.st);
}

// Block cokriging: the members on the device in both forms the kernels read (the site transform that prepares the centres), their
// weights and offsets, and the r prior variances sigma_BB through the joint block predictor's pair sum (ck_blocks.hip: pieces
// of CK_PRIOR_PIECE pairs, a fixed-order sum).  Fills the member fields of *P.  One synchronisation; *prior_ms: the device
// window of the pass ([ev0, ev1], free again behind the counting pass).
static int local_block_members(ck_handle* h, DevTemps& tmp, int i, const CkLocalBlockLayout& lay, int64_t r, CkLocalProblem* P,
                               double* prior_ms) {
    const int64_t bm = lay.mpad;
    double *d_xy = nullptr, *d_mc = nullptr, *d_mu = nullptr, *d_w = nullptr, *d_sbb = nullptr, *d_part = nullptr;
    int* d_bo = nullptr;
    long long* d_poff = nullptr;
    HIPCHK(tmp.get(&d_xy, (size_t)(2 * bm * 8)));
    HIPCHK(tmp.get(&d_mc, (size_t)(3 * bm * 8)));
    HIPCHK(tmp.get(&d_mu, (size_t)(3 * bm * 8)));
    HIPCHK(tmp.get(&d_w, (size_t)(bm * 8)));
    HIPCHK(tmp.get(&d_bo, ((size_t)r + 1) * sizeof(int)));
    HIPCHK(tmp.get(&d_sbb, (size_t)r * 8));
    std::vector<long long> poff;
    const int64_t n_pieces = ck_host_prior_pieces(lay.off.data(), (int32_t)r, 0, poff);
    HIPCHK(tmp.get(&d_poff, poff.size() * sizeof(long long)));
    HIPCHK(tmp.get(&d_part, (size_t)n_pieces * 8));
    HIPCHK(hipMemcpyAsync(d_xy, lay.xy.data(), (size_t)(2 * bm * 8), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_w, lay.w.data(), (size_t)(bm * 8), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_bo, lay.off.data(), ((size_t)r + 1) * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_poff, poff.data(), poff.size() * sizeof(long long), hipMemcpyHostToDevice, h->stream));
    ck_launch_prep_sites(h->stream, d_xy, bm, h->metric, d_mc, d_mc + bm, d_mc + 2 * bm, d_mu);
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    ck_launch_block_prior(h->stream, h->d_blk + 2 * i, h->metric, d_mc, d_mc + bm, d_mc + 2 * bm, d_w, d_bo, r, 0, d_poff, n_pieces,
                          d_part, d_sbb, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipEventSynchronize(h->ev1));   // poff is host memory
    HIPCHK(elapsed_ms(h->ev0, h->ev1, prior_ms));
    P->bo = d_bo;
    P->mc = d_mc;
    P->mu = d_mu;
    P->bw = d_w;
    P->sbb = d_sbb;
    P->bmpad = bm;
    return 0;
}

// The pair form's extras (ck_predict_local_pair); null: one process.  The call runs as process 0 (with cv = 0 the search does
// not look at the process); pred / pred_err are process 0's, these are process 1's and the covariance of the two errors.
struct LocalPair {
    double *pred1, *err1;
    double* cov;   // m or null
};

static int predict_local_impl(ck_handle* h, int i, const double* pcoords, int64_t m, double max_dist, int cv, double* pred,
                              double* pred_err, LocalResult* res, const LocalUniv* u, const LocalVecchia* vc = nullptr,
                              const LocalBlocks* bk = nullptr, const LocalWithhold* wh = nullptr, const LocalPair* pr = nullptr) {
    LocalResult& R = *res = LocalResult();
    if (ensure_layout(h, false)) return -1;   // sites, tables, chunk bounds -- no Sigma panels
    if (i < 0 || i >= h->n_procs) return fail("process index out of range");
    if (m < 0 || (m > 0 && !pcoords)) return fail("bad pcoords");
    if (m == 0) return 0;
    const auto t_begin = std::chrono::steady_clock::now();
    const int up = u ? trend_total(h) : 0;   // trend rows of every local system
    const int upi = u ? h->trend_p[i] : 0;
    if (u && ensure_trend(h)) return -1;
    if (ensure_noise(h)) return -1;
    const int64_t mp = roundup(m, 64);
    DevTemps tmp;
    double *d_out = nullptr, *d_slab = nullptr, *d_vv = nullptr;
    long long *d_off = nullptr, *d_linfo = nullptr;
    int* d_k0 = nullptr;
    CkLocalSys* d_sys = nullptr;
    HIPCHK(tmp.get(&d_out, (size_t)((pr ? 5 : 2) * mp * 8)));
    HIPCHK(tmp.get(&d_off, (size_t)(mp * sizeof(long long))));
    if (vc) {
        HIPCHK(tmp.get(&d_vv, (size_t)(mp * 8)));
        HIPCHK(hipMemsetAsync(d_vv, 0, (size_t)(mp * 8), h->stream));
    }
    // universal form: the regressors of the prediction points (a point with a non-finite one is settled on the host at the
    // end and computes with zeros meanwhile), the status of every point, the local coefficients
    double *d_f0 = nullptr, *d_beta = nullptr;
    int* d_stat = nullptr;
    std::vector<char> f0_bad;
    if (u) {
        std::vector<double> f0s((size_t)(m * upi));
        f0_bad.assign((size_t)m, 0);
        for (int64_t e = 0; e < m * upi; ++e) {
            const bool ok = std::isfinite(u->f0[e]);
            f0s[(size_t)e] = ok ? u->f0[e] : 0.0;
            if (!ok) f0_bad[(size_t)(e / upi)] = 1;
        }
        HIPCHK(tmp.get(&d_f0, (size_t)(m * upi * 8)));
        HIPCHK(tmp.get(&d_stat, (size_t)(mp * sizeof(int))));
        if (u->beta) HIPCHK(tmp.get(&d_beta, (size_t)(m * up * 8)));
        if (upi > 0) HIPCHK(hipMemcpy(d_f0, f0s.data(), (size_t)(m * upi * 8), hipMemcpyHostToDevice));
    }
    const CkLocalTrend Tr{h->d_trendX, d_f0, u ? h->trend_p[0] : 0, u && h->n_procs == 2 ? h->trend_p[1] : 0, CK_TREND_TOL};
    // the neighbour cap (ck_set_local_neighbours): the select pass replaces the counting pass and leaves every point's cut
    // distances and culling chord for the later launches; no cap: none of this exists and no kernel sees a new pointer.  The
    // host-side planning and a growth of the scratch slab (hipMalloc: up to seconds) lie between the pass and the solve window
    const bool select = local_nmax_of(h, 0) > 0 || local_nmax_of(h, 1) > 0 || vc;
    LocalPass S;
    if (local_pass(h, tmp, i, pcoords, m, max_dist, cv, select, vc ? vc->d_rs : nullptr, vc ? vc->rp : nullptr, nullptr, &S, wh)) return -1;
    if (bk && local_block_members(h, tmp, i, *bk->lay, m, &S.prob, &R.prior_ms)) return -1;
    const CkLocalProblem& P = S.prob;   // what every launch below is told about the call
    const int* d_cnt = S.d_cnt;
    const std::vector<int>& cnt = S.cnt;
    const double c0var = P.c0var;
    R.pass_ms = S.pass_ms;
    R.st = S.st;
    // Scratch slabs for neighbourhoods beyond the LDS limit.  Three size classes:
    //   k <= LDS limit               k_local_solve, system in LDS
    //   k <= local_tile_min          k_local_solve_big, one workgroup per point on a slab in global memory
    //   larger                       the tiled path (ck_internal.h: CkLocalSys): a batch of systems factored
    //                                together, three launches per 64 columns, updates on the MFMA tiles
    // Both slab users work in batches that fit a budget (a quarter of the free device memory, at most 32 GiB),
    // so that large radii over many points do not need sum_p k_p^2 doubles at once.
    const int kl = ck_local_lds_limit();
    // may lie below the LDS limit: then the LDS kernel only sees k <= k_hi.  The universal form has no slab kernel: every
    // neighbourhood beyond the LDS limit takes the tiled path
    const int k_hi = (u || bk || pr) ? std::min(h->local_tile_min, kl) : h->local_tile_min;
    const int xr = pr ? CK_LOCAL_PAIR_ROWS - 2 : up;   // rows of every tiled system beyond c and z
    CkLocalNeeds nd;   // ck_host.cpp: the slab need of every point, the tiled class largest first
    if (pr)
        ck_host_local_pair_needs(cnt.data(), m, kl, h->local_tile_min, &nd);
    else
        ck_host_local_needs(cnt.data(), m, kl, k_hi, up, &nd);
    long long budget = 0;
    size_t mem_free = 0;
    if (local_budget_doubles(h, &budget, &mem_free)) return -1;
    if (budget < nd.need_max) budget = nd.need_max;
    if ((size_t)nd.need_max * 8 > mem_free) return fail(std::string(pr ? "ck_predict_local_pair" : wh ? "ck_cv_local_folds" : bk ? "ck_predict_local_blocks" : u ? "ck_predict_local_universal" : "ck_predict_local") + ": a neighbourhood of " + std::to_string(nd.k_max) + " sites does not fit the device memory");
    CkLocalPlan plan;   // slab offsets, the batches of both classes under the budget, the tiled systems
    ck_host_local_plan(cnt.data(), nd, budget, xr, &plan);
    if (local_slab_grow(h, plan.slab_doubles, budget, &R.grow_ms)) return -1;
    if (plan.slab_doubles > 0) d_slab = h->local_slab;
    HIPCHK(hipEventRecord(h->ev2, h->stream));
    HIPCHK(hipMemcpyAsync(d_off, plan.off.data(), m * sizeof(long long), hipMemcpyHostToDevice, h->stream));
    const CkLocalPairOut PO{d_out,
                            d_out + mp,
                            d_out + 2 * mp,
                            d_out + 3 * mp,
                            d_out + 4 * mp,
                            {h->blk[0].amp + h->blk[0].nugget, h->blk[2].amp + h->blk[2].nugget},
                            ck_cov_entry(h->blk[1], 0.0, 0)};
    if (pr)   // the pair form: the LDS class here, everything larger on the tiled path below
        ck_launch_local_solve_pair(h->stream, P, m, d_cnt, k_hi, PO);
    else if (bk)   // the universal form's two classes, with or without a trend
        ck_launch_local_solve_b(h->stream, P, m, d_cnt, k_hi, Tr, d_out, d_out + mp, d_beta, d_stat);
    else if (u)
        ck_launch_local_solve_u(h->stream, P, m, d_cnt, k_hi, Tr, d_out, d_out + mp, d_beta, d_stat);
    else
        for (const auto& bt : plan.batches)
            ck_launch_local_solve(h->stream, P, bt.first, bt.second - bt.first, d_cnt, d_off, d_slab, k_hi, d_out, d_out + mp,
                                  d_vv);
    HIPCHK(hipGetLastError());
    std::vector<hipEvent_t> ev_red;   // universal form: an event pair around every batch's reduction (ck_timings [50])
    struct EvFree {
        std::vector<hipEvent_t>& v;
        ~EvFree() {
            for (hipEvent_t e : v) (void)hipEventDestroy(e);
        }
    } ev_free{ev_red};
    std::vector<hipEvent_t> ev_cls;   // block form: the end of the LDS class's launch (ck_timings [105] / [106])
    EvFree ev_free_cls{ev_cls};
    if (bk) {
        hipEvent_t e = nullptr;
        HIPCHK(hipEventCreate(&e));
        ev_cls.push_back(e);
        HIPCHK(hipEventRecord(e, h->stream));
    }
    if (!nd.tiled.empty()) {
        HIPCHK(tmp.get(&d_sys, (size_t)(plan.sys.size() * sizeof(CkLocalSys))));
        HIPCHK(tmp.get(&d_linfo, (size_t)(plan.sys.size() * sizeof(long long))));
        HIPCHK(tmp.get(&d_k0, (size_t)(plan.sys.size() * sizeof(int))));
        HIPCHK(hipMemcpyAsync(d_sys, plan.sys.data(), plan.sys.size() * sizeof(CkLocalSys), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemsetAsync(d_linfo, 0, plan.sys.size() * sizeof(long long), h->stream));
        for (const auto& tb : plan.tbatches) {
            const CkLocalSys* bsys = d_sys + tb.first;
            const int nb = (int)(tb.second - tb.first);
            ck_launch_local_assemble_t(h->stream, P, bsys, nb, d_slab, d_k0 + tb.first, pr != nullptr);
            if (u) ck_launch_local_trend_rows_t(h->stream, bsys, nb, d_slab, layout_of(h), Tr);
            const int kq_max = plan.sys[tb.first].kq;
            std::vector<int> kqv(nb);
            for (int y = 0; y < nb; ++y) kqv[y] = plan.sys[tb.first + y].kq;
            factor_tiled_batch(h->stream, bsys, d_slab, nb, kqv.data(), kq_max, kq_max, h->local_group,
                               h->local_left != 0 && 64 * h->local_group <= 256, d_linfo + tb.first);
            if (pr) {
                ck_launch_local_reduce_pair_t(h->stream, bsys, nb, d_slab, d_linfo + tb.first, PO);
            } else if (u) {
                hipEvent_t e0 = nullptr, e1 = nullptr;
                HIPCHK(hipEventCreate(&e0));
                ev_red.push_back(e0);
                HIPCHK(hipEventCreate(&e1));
                ev_red.push_back(e1);
                HIPCHK(hipEventRecord(e0, h->stream));
                ck_launch_local_reduce_ut(h->stream, bsys, nb, d_slab, d_linfo + tb.first, d_k0 + tb.first, i, c0var, d_out,
                                          d_out + mp, Tr, d_beta, d_stat, P.sbb);
                HIPCHK(hipEventRecord(e1, h->stream));
            } else {
                ck_launch_local_reduce_t(h->stream, bsys, nb, d_slab, d_linfo + tb.first, c0var, d_out, d_out + mp, d_vv, P.sbb);
            }
            HIPCHK(hipGetLastError());
        }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev3, h->stream));
    HIPCHK(hipMemcpyAsync(pred, d_out, m * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(pred_err, d_out + mp, m * 8, hipMemcpyDeviceToHost, h->stream));
    if (pr) {
        HIPCHK(hipMemcpyAsync(pr->pred1, PO.pred1, m * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(pr->err1, PO.err1, m * 8, hipMemcpyDeviceToHost, h->stream));
        if (pr->cov) HIPCHK(hipMemcpyAsync(pr->cov, PO.cov, m * 8, hipMemcpyDeviceToHost, h->stream));
    }
    if (vc) {
        HIPCHK(hipMemcpyAsync(vc->vv, d_vv, m * 8, hipMemcpyDeviceToHost, h->stream));
        for (int64_t p = 0; p < m; ++p) {
            vc->cnt2[2 * p] = S.sel[(size_t)(4 * p)];
            vc->cnt2[2 * p + 1] = S.sel[(size_t)(4 * p + 1)];
        }
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(elapsed_ms(h->ev2, h->ev3, &R.solve_ms));
    R.k_max = nd.k_max;
    R.n_tiled = (int64_t)nd.tiled.size();
    R.n_tbatches = nd.tiled.empty() ? 0 : (int64_t)plan.tbatches.size();
    R.n_empty = nd.n_empty;
    if (bk) {
        double t = 0;
        HIPCHK(elapsed_ms(h->ev2, ev_cls[0], &t));
        R.lds_ms = t;
        for (int64_t b = 0; b < m; ++b)
            R.cbar_evals += (double)(bk->lay->off[(size_t)b + 1] - bk->lay->off[(size_t)b]) * (double)cnt[(size_t)b];
        R.total_ms = ms_since(t_begin);
    }
    if (u) {
        std::vector<int> stat((size_t)m);
        HIPCHK(hipMemcpy(stat.data(), d_stat, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
        if (u->beta) HIPCHK(hipMemcpy(u->beta, d_beta, (size_t)(m * up * 8), hipMemcpyDeviceToHost));
        int64_t nrd = 0;
        R.n_empty = 0;
        for (int64_t p = 0; p < m; ++p) {
            if (f0_bad[(size_t)p]) {   // rule 5: NaN, in none of the counters
                pred[p] = pred_err[p] = NAN;
                if (u->beta)
                    for (int j = 0; j < up; ++j) u->beta[p * up + j] = NAN;
                continue;
            }
            R.n_empty += stat[(size_t)p] == CK_LU_EMPTY;
            R.n_not_pd += stat[(size_t)p] == CK_LU_NOT_PD;
            nrd += stat[(size_t)p] == CK_LU_RANK_DEF;
        }
        if (u->n_rank_def) *u->n_rank_def = nrd;
        for (size_t e = 0; e + 1 < ev_red.size(); e += 2) {
            double t = 0;
            HIPCHK(elapsed_ms(ev_red[e], ev_red[e + 1], &t));
            R.reduce_ms += t;
        }
        R.total_ms = ms_since(t_begin);
    } else {
        for (int64_t p = 0; p < m; ++p)
            if (cnt[(size_t)p] > 0 && pred[p] != pred[p]) ++R.n_not_pd;
    }
    return 0;
}

// The exported predictions: the counts to the caller (any may be null), then the call's ck_timings slots, once.  m = 0: no
// call ran and the slots of ck_predict_local keep what they held.
static void local_counts_out(const LocalResult& R, int64_t* n_empty, int64_t* n_not_pd, int64_t* k_max) {
    if (n_empty) *n_empty = R.n_empty;
    if (n_not_pd) *n_not_pd = R.n_not_pd;
    if (k_max) *k_max = R.k_max;
}

extern "C" int ck_predict_local(ck_handle* h, int i, const double* pcoords, int64_t m, double max_dist, int cv,
                                double* pred, double* pred_err, int64_t* n_empty, int64_t* n_not_pd,
                                int64_t* k_max) {
    CHKH(h);
    LocalResult R;
    if (predict_local_impl(h, i, pcoords, m, max_dist, cv, pred, pred_err, &R, nullptr)) return -1;
    local_counts_out(R, n_empty, n_not_pd, k_max);
    if (m > 0) write_local_timings(h, R);
    return 0;
}

// Universal cokriging in the moving neighbourhood: include/cokrige.h has the arithmetic and the rules for degenerate cases;
// ck_local.hip the kernels.  No trend set: ck_predict_local itself.
extern "C" int ck_predict_local_universal(ck_handle* h, int i, const double* pcoords, int64_t m, const double* f0, double max_dist,
                                          int cv, double* pred, double* pred_err, double* beta, int64_t* n_empty,
                                          int64_t* n_not_pd, int64_t* n_rank_def, int64_t* k_max) {
    CHKH(h);
    if (h->world != 1)
        return fail("ck_predict_local_universal is the single-process form: this handle is partitioned (world = " +
                    std::to_string(h->world) + ")");
    if (n_rank_def) *n_rank_def = 0;
    if (i < 0 || i >= h->n_procs) return fail("process index out of range");
    if (m > 0 && (!pred || !pred_err)) return fail("ck_predict_local_universal: bad prediction arrays");
    timings_from(h, 48);
    const bool trend = trend_total(h) > 0;
    if (trend && m > 0 && h->trend_p[i] > 0 && !f0) return fail("ck_predict_local_universal: null regressors of the prediction sites");
    const LocalUniv u{f0, beta, n_rank_def};
    LocalResult R;
    if (predict_local_impl(h, i, pcoords, m, max_dist, cv, pred, pred_err, &R, trend ? &u : nullptr)) return -1;
    local_counts_out(R, n_empty, n_not_pd, k_max);
    if (m > 0) write_local_timings(h, R);
    if (m > 0 && trend) {
        h->t_ms[48] = R.pass_ms;                      // the counting pass
        h->t_ms[49] = R.solve_ms - R.reduce_ms;       // assembly and factorisation (the LDS class's kernel whole)
        h->t_ms[50] = R.reduce_ms;                    // the tiled class's universal reduction (Gram matrix + GLS step)
        h->t_ms[51] = R.total_ms;
        h->t_ms[52] = (double)(m - R.n_tiled);        // points of the LDS class (the empty ones among them)
        h->t_ms[53] = (double)R.n_tiled;              // points of the tiled class
    }
    return 0;
}

// Block cokriging in the moving neighbourhood: include/cokrige.h has the definition; ck_host.cpp the member layout, ck_local.hip
// the kernels.  The stages are predict_local_impl's, run on the blocks' centres.
extern "C" int ck_predict_local_blocks(ck_handle* h, int i, const double* centres, int32_t r, const double* pcoords, int64_t m,
                                       const int32_t* block, const double* weight, const double* f0, double max_dist, double* pred,
                                       double* pred_err, double* beta, int64_t* n_empty, int64_t* n_not_pd, int64_t* n_rank_def,
                                       int64_t* k_max) {
    CHKH(h);
    if (h->world != 1)
        return fail("ck_predict_local_blocks is the single-process form: this handle is partitioned (world = " +
                    std::to_string(h->world) + ")");
    if (n_rank_def) *n_rank_def = 0;
    if (i < 0 || i >= h->n_procs) return fail("process index out of range");
    if (!centres || !pcoords || !block || !weight || !pred || !pred_err) return fail("ck_predict_local_blocks: null argument");
    const bool trend = trend_total(h) > 0;
    if (trend && h->trend_p[i] > 0 && !f0)
        return fail("ck_predict_local_blocks: null block regressors f0 with a trend of p_i = " + std::to_string(h->trend_p[i]) +
                    " columns of process " + std::to_string(i));
    CkLocalBlockLayout lay;
    if (ck_host_local_block_layout(centres, r, pcoords, m, block, weight, 64, &lay)) return -1;
    timings_from(h, 104);
    const LocalUniv u{f0, beta, n_rank_def};
    const LocalBlocks bk{&lay};
    LocalResult R;
    if (predict_local_impl(h, i, centres, r, max_dist, 0, pred, pred_err, &R, trend ? &u : nullptr, nullptr, &bk)) return -1;
    local_counts_out(R, n_empty, n_not_pd, k_max);
    write_local_timings(h, R);
    h->t_ms[104] = R.pass_ms;                    // the counting or select pass of the centres
    h->t_ms[105] = R.n_tiled ? R.lds_ms : R.solve_ms;           // the LDS class: search, assembly with cbar, factorisation, outputs
    h->t_ms[106] = R.n_tiled ? R.solve_ms - R.lds_ms : 0.0;     // the tiled class (0: no block took it)
    h->t_ms[107] = R.prior_ms;                   // the sigma_BB pass
    h->t_ms[108] = R.total_ms;                   // host wall clock of the call
    h->t_ms[109] = R.cbar_evals;                 // sum_b q_b k_b
    return 0;
}

// Both processes at every point from one local system: include/cokrige.h has the definition; ck_host.cpp the size classes with
// three extra rows, ck_local.hip the kernels.  The stages are predict_local_impl's, run as process 0.
extern "C" int ck_predict_local_pair(ck_handle* h, const double* pcoords, int64_t m, double max_dist, double* pred0, double* pred_err0,
                                     double* pred1, double* pred_err1, double* pred_cov, int64_t* n_empty, int64_t* n_not_pd,
                                     int64_t* k_max) {
    CHKH(h);
    const std::string name = "ck_predict_local_pair";
    if (h->world != 1)
        return fail(name + " is the single-process form: this handle is partitioned (world = " + std::to_string(h->world) + ")");
    if (!h->model_set || h->n_procs != 2)
        return fail(name + ": needs a model of two processes (n_procs = " + std::to_string(h->n_procs) + ")");
    if (trend_total(h) > 0)
        return fail(name + ": a trend of " + std::to_string(trend_total(h)) +
                    " columns is set on the handle; the pair form takes none (clear it with ck_set_trend)");
    if (m < 1) return fail(name + ": m = " + std::to_string(m) + " points; at least 1");
    if (!(max_dist >= 0.0) || !std::isfinite(max_dist))
        return fail(name + ": max_dist must be finite and >= 0, got " + std::to_string(max_dist));
    if (!pcoords || !pred0 || !pred_err0 || !pred1 || !pred_err1 || !n_empty || !n_not_pd || !k_max)
        return fail(name + ": null pcoords_host / pred0 / pred_err0 / pred1 / pred_err1 / n_empty / n_not_pd / k_max");
    timings_from(h, 138);
    const LocalPair pr{pred1, pred_err1, pred_cov};
    LocalResult R;
    if (predict_local_impl(h, 0, pcoords, m, max_dist, 0, pred0, pred_err0, &R, nullptr, nullptr, nullptr, nullptr, &pr)) return -1;
    local_counts_out(R, n_empty, n_not_pd, k_max);
    write_select_timings(h, R.st);        // [60 .. 63], as after every local call
    h->t_ms[138] = R.pass_ms;             // the counting pass (a capped call's select pass)
    h->t_ms[139] = R.solve_ms;            // the solve window: both classes' assembly, factorisation and outputs
    h->t_ms[140] = R.grow_ms;             // host: a growth of the scratch slab
    h->t_ms[141] = (double)R.n_tiled;     // points of the tiled class
    h->t_ms[142] = (double)R.n_tbatches;  // batches they were factored in (the slab budget)
    return 0;
}

// ---------------------------------------------------------------------------------------
// leave-group-out and buffer cross-validation in the moving neighbourhood (include/cokrige.h has the rules)
// ---------------------------------------------------------------------------------------
// What ck_cv_local_folds and ck_debug_local_cv_neighbours (name) do before the first launch, written once: the refusals, the layout,
// the plan (ck_host.cpp), the labels of both processes in the internal site order on the device (k_cv_labels; null without
// labels) and the coordinates of the predicted data.
struct LocalCvStages {
    CkLocalCvPlan plan;
    LocalWithhold wh{nullptr, nullptr, {-1.0, -1.0}};
    std::vector<double> pts;   // m x 2: the predicted data's coordinates, plist order
    int64_t m = 0;
};
static int local_cv_stages(ck_handle* h, const std::string& name, int i, const int32_t* fold0, const int32_t* fold1, int32_t n_folds,
                           const double* buffer2, double max_dist, DevTemps& tmp, LocalCvStages* out) {
    LocalCvStages& C = *out;
    if (h->world != 1)
        return fail(name + " is the single-process form: this handle is partitioned (world = " + std::to_string(h->world) + ")");
    if (i < 0 || i >= h->n_procs) return fail(name + ": process index " + std::to_string(i) + " out of range");
    if (!(max_dist >= 0.0) || !std::isfinite(max_dist))
        return fail(name + ": max_dist must be finite and >= 0, got " + std::to_string(max_dist));
    for (int q = 0; q < 2 && buffer2; ++q) {
        if (!std::isfinite(buffer2[q])) return fail(name + ": buffer2[" + std::to_string(q) + "] = " + std::to_string(buffer2[q]) + " is not finite (a negative value turns the buffer of a process off)");
        C.wh.wb[q] = q < h->n_procs && buffer2[q] >= 0.0 ? buffer2[q] : -1.0;
    }
    if (ensure_layout(h, false)) return -1;   // sites, tables, chunk bounds, perm -- no Sigma panels
    if (h->N > INT32_MAX) return fail(name + ": more than 2^31 - 1 data");
    if (ck_host_local_cv_plan(name.c_str(), i, h->n_procs, h->n, h->n0p, h->perm[0].data(), h->n_procs == 2 ? h->perm[1].data() : nullptr,
                              fold0, fold1, n_folds, C.wh.wb[i] >= 0.0, &C.plan))
        return -1;
    const int32_t* fold[2] = {fold0, h->n_procs == 2 ? fold1 : nullptr};
    const int64_t n0 = h->n[0], n1 = h->n_procs == 2 ? h->n[1] : 0;
    if (n_folds > 0 && (fold[0] || fold[1])) {
        int *d_fs = nullptr, *d_lab = nullptr, *d_gself = nullptr;
        HIPCHK(tmp.get(&d_fs, (size_t)h->Npad * sizeof(int)));
        HIPCHK(tmp.get(&d_lab, (size_t)std::max<int64_t>(h->N, 1) * sizeof(int)));
        HIPCHK(tmp.get(&d_gself, (size_t)std::max<int64_t>(h->N, 1) * sizeof(int)));
        HIPCHK(hipMemsetAsync(d_fs, 0xFF, (size_t)h->Npad * sizeof(int), h->stream));   // -1 everywhere
        if (fold[0] && n0 > 0) HIPCHK(hipMemcpyAsync(d_lab, fold[0], (size_t)n0 * sizeof(int), hipMemcpyHostToDevice, h->stream));
        if (fold[1] && n1 > 0) HIPCHK(hipMemcpyAsync(d_lab + n0, fold[1], (size_t)n1 * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(d_gself, C.plan.gself.data(), (size_t)h->N * sizeof(int), hipMemcpyHostToDevice, h->stream));
        ck_launch_cv_labels(h->stream, n0, n1, fold[0] ? d_lab : nullptr, fold[1] ? d_lab + n0 : nullptr, d_gself, d_fs);
        HIPCHK(hipGetLastError());
        C.wh.d_fs = d_fs;
        C.wh.fp = C.plan.fp.data();
    }
    C.m = (int64_t)C.plan.plist.size();
    C.pts.resize((size_t)(2 * C.m));
    for (int64_t t = 0; t < C.m; ++t) {
        const int64_t a = C.plan.plist[(size_t)t];
        C.pts[(size_t)(2 * t)] = h->h_coords[i][(size_t)(2 * a)];
        C.pts[(size_t)(2 * t + 1)] = h->h_coords[i][(size_t)(2 * a + 1)];
    }
    return 0;
}

// The select pass of a cross-validation call alone, with the handle's caps: the test surface of the withholding conditions.
extern "C" int ck_debug_local_cv_neighbours(ck_handle* h, int i, const int32_t* fold0, const int32_t* fold1, int32_t n_folds,
                                            const double* buffer2, double max_dist, int32_t* count, double* rcut) {
    CHKH(h);
    const std::string name = "ck_debug_local_cv_neighbours";
    if (i >= 0 && i < h->n_procs && h->n[i] > 0 && (!count || !rcut)) return fail(name + ": null count / rcut");
    DevTemps tmp;
    LocalCvStages C;
    if (local_cv_stages(h, name, i, fold0, fold1, n_folds, buffer2, max_dist, tmp, &C)) return -1;
    timings_from(h, 60);
    LocalPass S;
    std::vector<double> rc((size_t)(2 * C.m));
    if (C.m > 0 && local_pass(h, tmp, i, C.pts.data(), C.m, max_dist, 0, true, nullptr, nullptr, rc.data(), &S, &C.wh)) return -1;
    for (int64_t a = 0; a < 2 * h->n[i]; ++a) {
        count[a] = 0;
        rcut[a] = NAN;
    }
    for (int64_t t = 0; t < C.m; ++t) {
        const int64_t a = C.plan.plist[(size_t)t];
        for (int q = 0; q < 2; ++q) {
            count[2 * a + q] = S.sel[(size_t)(4 * t + q)];
            rcut[2 * a + q] = rc[(size_t)(2 * t + q)];
        }
    }
    write_select_timings(h, S.st);
    return 0;
}

extern "C" int ck_cv_local_folds(ck_handle* h, int i, const int32_t* fold0, const int32_t* fold1, int32_t n_folds, const double* buffer2,
                                 const double* f0, double max_dist, double* pred, double* pred_err, double* beta, double* fold_stats,
                                 double* score5, int64_t* counters4) {
    CHKH(h);
    const std::string name = "ck_cv_local_folds";
    const auto t_begin = std::chrono::steady_clock::now();
    if (i >= 0 && i < h->n_procs && h->n[i] > 0 && (!pred || !pred_err)) return fail(name + ": null pred / pred_err");
    const bool trend = trend_total(h) > 0;
    if (trend && i >= 0 && i < h->n_procs && h->trend_p[i] > 0 && !f0)
        return fail(name + ": null regressors f0 with a trend of p_i = " + std::to_string(h->trend_p[i]) + " columns of process " +
                    std::to_string(i));
    DevTemps tmp;
    LocalCvStages C;
    if (local_cv_stages(h, name, i, fold0, fold1, n_folds, buffer2, max_dist, tmp, &C)) return -1;
    timings_from(h, 118);
    const int64_t m = C.m, n_i = h->n[i];
    const int up = trend ? trend_total(h) : 0, upi = trend ? h->trend_p[i] : 0;
    // the predicted data are the points of one call of the local predictor; its outputs come back in plist order
    std::vector<double> pl((size_t)m), el((size_t)m), f0l((size_t)(m * upi)), bl(beta ? (size_t)(m * up) : 0);
    for (int64_t t = 0; t < m; ++t)
        for (int j = 0; j < upi; ++j) f0l[(size_t)(t * upi + j)] = f0[(int64_t)C.plan.plist[(size_t)t] * upi + j];
    int64_t n_rank_def = 0;
    const LocalUniv u{f0l.data(), beta ? bl.data() : nullptr, &n_rank_def};
    LocalResult R;
    if (predict_local_impl(h, i, C.pts.data(), m, max_dist, 0, pl.data(), el.data(), &R, trend ? &u : nullptr, nullptr, nullptr, &C.wh))
        return -1;
    for (int64_t a = 0; a < n_i; ++a) pred[a] = pred_err[a] = NAN;
    if (beta) std::fill(beta, beta + n_i * up, NAN);
    for (int64_t t = 0; t < m; ++t) {
        const int64_t a = C.plan.plist[(size_t)t];
        pred[a] = pl[(size_t)t];
        pred_err[a] = el[(size_t)t];
        for (int j = 0; beta && j < up; ++j) beta[a * up + j] = bl[(size_t)(t * up + j)];
    }
    if (counters4) {
        counters4[0] = R.n_empty;
        counters4[1] = R.n_not_pd;
        counters4[2] = n_rank_def;
        counters4[3] = R.k_max;
    }
    // the scores: e = z - pred, v = pred_err^2 + the datum's own s d (the variance of the withheld OBSERVATION), one workgroup
    // per group of the plan, then the totals over the groups in order on the host
    const int64_t ng = C.plan.n_groups;
    std::vector<double> sums((size_t)(ng * CK_CV_NSCORE), 0.0);
    double scores_ms = 0.0;
    if (m > 0 && ng > 0 && (fold_stats || score5)) {
        const bool nz = h->noise_on && !h->noise_var[i].empty();
        std::vector<double> zl((size_t)m), ol(nz ? (size_t)m : 0);
        for (int64_t t = 0; t < m; ++t) {
            const int64_t a = C.plan.plist[(size_t)t];
            zl[(size_t)t] = h->h_values[i][(size_t)a];
            if (nz) ol[(size_t)t] = h->noise_scale[i] * h->noise_var[i][(size_t)a];
        }
        double *d_in = nullptr, *d_sum = nullptr;
        int* d_idx = nullptr;
        long long* d_goff = nullptr;
        HIPCHK(tmp.get(&d_in, (size_t)(4 * m * 8)));
        HIPCHK(tmp.get(&d_sum, (size_t)(ng * CK_CV_NSCORE * 8)));
        HIPCHK(tmp.get(&d_idx, (size_t)m * sizeof(int)));
        HIPCHK(tmp.get(&d_goff, (size_t)(ng + 1) * sizeof(long long)));
        HIPCHK(hipMemcpyAsync(d_in, zl.data(), (size_t)(m * 8), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(d_in + m, pl.data(), (size_t)(m * 8), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(d_in + 2 * m, el.data(), (size_t)(m * 8), hipMemcpyHostToDevice, h->stream));
        if (nz) HIPCHK(hipMemcpyAsync(d_in + 3 * m, ol.data(), (size_t)(m * 8), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(d_idx, C.plan.idx.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(d_goff, C.plan.off.data(), (size_t)(ng + 1) * sizeof(long long), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipEventRecord(h->ev0, h->stream));
        ck_launch_cv_fold_scores(h->stream, ng, CkCvScoreArgs{d_idx, d_goff, d_in, d_in + m, d_in + 2 * m, nz ? d_in + 3 * m : nullptr, d_sum});
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->ev1, h->stream));
        HIPCHK(hipMemcpyAsync(sums.data(), d_sum, sums.size() * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(elapsed_ms(h->ev0, h->ev1, &scores_ms));
    }
    if (fold_stats)
        for (int32_t f = 0; f < n_folds; ++f) {
            fold_stats[6 * f] = (double)C.plan.size[(size_t)f];
            for (int c = 0; c < CK_CV_NSCORE; ++c) fold_stats[6 * f + 1 + c] = sums[(size_t)(f * CK_CV_NSCORE + c)];
        }
    if (score5)
        for (int c = 0; c < CK_CV_NSCORE; ++c) {
            double acc = 0.0;
            for (int64_t g = 0; g < ng; ++g) acc += sums[(size_t)(g * CK_CV_NSCORE + c)];
            score5[c] = acc;
        }
    if (m > 0) write_local_timings(h, R);
    h->t_ms[118] = R.pass_ms;             // the counting or select pass of the predicted data
    h->t_ms[119] = R.solve_ms;            // assembly, factorisations, reductions: every size class
    h->t_ms[120] = scores_ms;             // k_cv_fold_scores
    h->t_ms[121] = ms_since(t_begin);     // host wall clock of the call
    h->t_ms[122] = (double)m;             // data predicted
    h->t_ms[123] = (double)n_folds;
    return 0;
}

// ---------------------------------------------------------------------------------------
// the Vecchia likelihood (include/cokrige.h has the definition)
// ---------------------------------------------------------------------------------------
// What the Vecchia entry points (name) refuse, in this order, before they touch the device; null_args: the arguments the
// entry point cannot do without, named when one of them is null; trend_ok: the entry point takes a trend (ck_loglik_vecchia_trend).  Then the layout: sites, tables, chunk bounds -- no Sigma
// panels, nothing invalidated.
static int vecchia_admit(ck_handle* h, const std::string& name, const char* null_args, double max_dist, bool trend_ok = false) {
    if (h->world != 1)
        return fail(name + " is the single-process form: this handle is partitioned (world = " + std::to_string(h->world) + ")");
    if (null_args) return fail(name + ": null " + null_args);
    if (!(max_dist >= 0.0) || !std::isfinite(max_dist))
        return fail(name + ": max_dist must be finite and >= 0, got " + std::to_string(max_dist));
    if (trend_total(h) > 0 && !trend_ok)
        return fail(name + ": a trend of " + std::to_string(trend_total(h)) +
                    " columns is set on the handle; the Vecchia likelihood has no REML form (clear it with ck_set_trend)");
    if (ensure_layout(h, false)) return -1;
    if (ensure_noise(h)) return -1;
    if (trend_ok && ensure_trend(h)) return -1;
    if (h->N > INT32_MAX) return fail(name + ": more than 2^31 - 1 data");
    return 0;
}
// The ordering: positions of the data and of the sites (ck_host.cpp), the sites' on the device for the precedence condition
static int vecchia_order(ck_handle* h, const std::string& name, const int64_t* rank_host, DevTemps& tmp, CkVecchiaOrder* ord,
                         int** d_rs) {
    if (ck_host_vecchia_order(rank_host, h->n_procs, h->n, h->n0p, h->Npad, h->perm[0].data(),
                              h->n_procs == 2 ? h->perm[1].data() : nullptr, ord))
        return fail(name + ": data " + std::to_string(ord->dup[0]) + " and " + std::to_string(ord->dup[1]) +
                    " (stacked order) have the same rank " + std::to_string((long long)rank_host[ord->dup[0]]));
    HIPCHK(tmp.get(d_rs, (size_t)h->Npad * sizeof(int)));
    HIPCHK(hipMemcpyAsync(*d_rs, ord->rs.data(), (size_t)h->Npad * sizeof(int), hipMemcpyHostToDevice, h->stream));
    return 0;
}

// The data as the terms need them, in the caller's stacked order: every datum's value, prior variance and own measurement-error
// variance s d (0 without noise)
struct VecchiaData {
    std::vector<double> zs, prior, own;
};
static void vecchia_data(const ck_handle* h, VecchiaData* D) {
    D->zs.resize((size_t)h->N);
    D->prior.resize((size_t)h->N);
    D->own.assign((size_t)h->N, 0.0);
    for (int k = 0; k < h->n_procs; ++k) {
        const int64_t soff = k == 0 ? 0 : h->n[0];
        const double c0 = h->blk[2 * k].amp + h->blk[2 * k].nugget;
        const bool nz = h->noise_on && !h->noise_var[k].empty();
        for (int64_t t = 0; t < h->n[k]; ++t) {
            D->prior[(size_t)(soff + t)] = c0;
            D->zs[(size_t)(soff + t)] = h->h_values[k][(size_t)t];
            if (nz) D->own[(size_t)(soff + t)] = h->noise_scale[k] * h->noise_var[k][(size_t)t];
        }
    }
}

// What a Vecchia call reports: stats3 to the caller, ck_timings [10], [14], [60 .. 63] and [72 .. 77] (the gradient then writes
// [80 .. 85])
struct VecchiaReport {
    int64_t n_empty = 0, k_max = 0, n_lds = 0, n_tiled = 0;
    LocalSelectStats st;   // over the passes of both processes
    double solve_ms = 0.0, grow_ms = 0.0, terms_ms = 0.0, total_ms = 0.0;
};
static void vecchia_report(ck_handle* h, const VecchiaReport& V, int64_t* stats3) {
    if (stats3) {
        stats3[0] = V.n_empty;
        stats3[1] = V.k_max;
        stats3[2] = V.st.n_capped;
    }
    h->t_ms[10] = V.st.ms + V.solve_ms;
    h->t_ms[14] = V.grow_ms;
    write_select_timings(h, V.st);
    h->t_ms[72] = V.st.ms;
    h->t_ms[73] = V.solve_ms;
    h->t_ms[74] = V.terms_ms;
    h->t_ms[75] = V.total_ms;
    h->t_ms[76] = (double)V.n_lds;
    h->t_ms[77] = (double)V.n_tiled;
}

// The terms and their sums in the caller's stacked order, from what the passes of the local solver left on the host: the tail of
// the Vecchia entry points -- the same uploads and launches, so the same bits in out3.  *terms_ms: the two term kernels
// ([ev0, ev1], read here).  rows (ck_loglik_vecchia_trend; null: none): the term kernel also writes every datum's row.
static int vecchia_terms_tail(ck_handle* h, DevTemps& tmp, const VecchiaData& D, const std::vector<double>& mu, std::vector<double>& vv,
                              const std::vector<int32_t>& cnt2, double* out3, double* mean_host, double* var_host,
                              int32_t* count_host, int64_t* info, int64_t* n_lds_out, double* terms_ms,
                              const CkVecchiaTrendRows* rows = nullptr) {
    const int64_t N = h->N;
    const int kl = ck_local_lds_limit();
    int64_t n_lds = 0;
    for (int64_t t = 0; t < N; ++t) {
        const int kt = cnt2[(size_t)(2 * t)] + cnt2[(size_t)(2 * t + 1)];
        n_lds += kt <= kl;
        if (kt > 0 && mu[(size_t)t] != mu[(size_t)t]) vv[(size_t)t] = NAN;   // not positive definite: no variance either
    }
    // the terms and their sums, in the caller's stacked order
    const int64_t nblk = (N + 255) / 256;
    double *d_z = nullptr, *d_mu = nullptr, *d_vv = nullptr, *d_prior = nullptr, *d_own = nullptr, *d_mean = nullptr, *d_var = nullptr,
           *d_part = nullptr, *d_out = nullptr;
    int* d_cnt2 = nullptr;
    long long* d_bad = nullptr;
    for (double** b : {&d_z, &d_mu, &d_vv, &d_prior, &d_own, &d_mean, &d_var}) HIPCHK(tmp.get(b, (size_t)(N * 8)));
    HIPCHK(tmp.get(&d_part, (size_t)(2 * nblk * 8)));
    HIPCHK(tmp.get(&d_out, (size_t)(2 * 8)));
    HIPCHK(tmp.get(&d_cnt2, (size_t)(2 * N) * sizeof(int)));
    HIPCHK(tmp.get(&d_bad, (size_t)(nblk + 1) * sizeof(long long)));
    const std::pair<double*, const double*> up[] = {{d_z, D.zs.data()}, {d_mu, mu.data()}, {d_vv, vv.data()}, {d_prior, D.prior.data()},
                                                    {d_own, D.own.data()}};
    for (const auto& c : up) HIPCHK(hipMemcpyAsync(c.first, c.second, (size_t)(N * 8), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_cnt2, cnt2.data(), (size_t)(2 * N) * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    if (rows)
        ck_launch_vecchia_trend_terms(h->stream, N, d_z, d_mu, d_vv, d_prior, h->noise_on ? d_own : nullptr, d_cnt2, *rows, d_mean,
                                      d_var, d_part, d_bad, d_out, d_bad + nblk);
    else
        ck_launch_vecchia_terms(h->stream, N, d_z, d_mu, d_vv, d_prior, h->noise_on ? d_own : nullptr, d_cnt2, d_mean, d_var, d_part,
                                d_bad, d_out, d_bad + nblk);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    double sums[2] = {0.0, 0.0};
    long long first_bad = 0;
    HIPCHK(hipMemcpyAsync(sums, d_out, 2 * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(&first_bad, d_bad + nblk, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    if (mean_host) HIPCHK(hipMemcpyAsync(mean_host, d_mean, (size_t)(N * 8), hipMemcpyDeviceToHost, h->stream));
    if (var_host) HIPCHK(hipMemcpyAsync(var_host, d_var, (size_t)(N * 8), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(elapsed_ms(h->ev0, h->ev1, terms_ms));
    if (count_host) memcpy(count_host, cnt2.data(), (size_t)(2 * N) * sizeof(int32_t));
    out3[1] = sums[0];
    out3[2] = sums[1];
    out3[0] = first_bad ? NAN : ck_vecchia_total(N, sums[0], sums[1]);
    if (first_bad) out3[1] = out3[2] = NAN;
    if (info) *info = first_bad;
    *n_lds_out = n_lds;
    return 0;
}

// The zero-mean value in an entry point's name (ck_loglik_vecchia; ck_loglik_vecchia_trend on a handle without a trend), behind
// vecchia_admit: both size classes of the local solver, then the terms.
static int vecchia_value(ck_handle* h, const std::string& name, const int64_t* rank_host, double max_dist, double* out3,
                         double* mean_host, double* var_host, int32_t* count_host, int64_t* stats3, int64_t* info) {
    const auto t_begin = std::chrono::steady_clock::now();
    timings_from(h, 72);
    const int64_t N = h->N;
    DevTemps tmp;
    CkVecchiaOrder ord;
    int* d_rs = nullptr;
    if (vecchia_order(h, name, rank_host, tmp, &ord, &d_rs)) return -1;
    // one pass of the local solver per process: its data are the points, i_pred = the process
    std::vector<double> mu((size_t)N), vv((size_t)N, 0.0), sd((size_t)N);
    std::vector<int32_t> cnt2((size_t)(2 * N), 0);
    VecchiaReport V;
    for (int k = 0; k < h->n_procs; ++k) {
        const int64_t nk = h->n[k], soff = k == 0 ? 0 : h->n[0];
        if (nk == 0) continue;
        const LocalVecchia vc{d_rs, ord.pos.data() + soff, vv.data() + soff, cnt2.data() + 2 * soff};
        LocalResult R;
        if (predict_local_impl(h, k, h->h_coords[k].data(), nk, max_dist, 0, mu.data() + soff, sd.data() + soff, &R, nullptr, &vc))
            return -1;
        V.n_empty += R.n_empty;
        V.k_max = std::max(V.k_max, R.k_max);
        V.st.add(R.st);
        V.solve_ms += R.solve_ms;
        V.grow_ms += R.grow_ms;
    }
    VecchiaData D;
    vecchia_data(h, &D);
    if (vecchia_terms_tail(h, tmp, D, mu, vv, cnt2, out3, mean_host, var_host, count_host, info, &V.n_lds, &V.terms_ms)) return -1;
    V.n_tiled = N - V.n_lds;
    V.total_ms = ms_since(t_begin);
    vecchia_report(h, V, stats3);
    return 0;
}

extern "C" int ck_loglik_vecchia(ck_handle* h, const int64_t* rank_host, double max_dist, double* out3, double* mean_host,
                                 double* var_host, int32_t* count_host, int64_t* stats3, int64_t* info) {
    CHKH(h);
    if (vecchia_admit(h, "ck_loglik_vecchia", rank_host && out3 ? nullptr : "rank_host / out3", max_dist)) return -1;
    return vecchia_value(h, "ck_loglik_vecchia", rank_host, max_dist, out3, mean_host, var_host, count_host, stats3, info);
}

// What the two calls on the LDS class of the local solver (name: ck_loglik_vecchia_grad, ck_loglik_vecchia_fisher) do before
// their own kernel, written once: the ordering, the live slots (ck_loglik_fisher's rule) and the operands of the pair rule
// (ck_loglik's), every datum's own internal index on the device, then the select pass of BOTH processes -- a set beyond the LDS
// limit is refused here, before any solve (refused_for: what the message says the call is for).
struct VecchiaLdsStages {
    CkVecchiaOrder ord;   // with every datum's own internal index (gself)
    int* d_rs = nullptr;
    CkVecchiaModel V{};
    const double* dvar = nullptr;   // the raw measurement-error variances, internal order; null: no noise slot is live
    int* d_gself = nullptr;
    LocalPass pass[2];              // a process's pass: the select here, the solve in the caller's kernel
    std::vector<int32_t> cnt2;
    VecchiaReport rep;
    int64_t n_pairs = 0, n_square = 0;   // sum over the data of (k + 1)(k + 2) / 2 and of (k + 1)^2
};
static int vecchia_lds_stages(ck_handle* h, const std::string& name, const char* refused_for, const int64_t* rank_host,
                              double max_dist, const int32_t* free13, DevTemps& tmp, VecchiaLdsStages* out) {
    static_assert(CK_FISHER_NPAR == CK_VG_NPAR, "the score has the slots of ck_loglik_fisher");
    VecchiaLdsStages& C = *out;
    const int64_t N = h->N, n0 = h->n[0], Np = h->Npad;
    if (vecchia_order(h, name, rank_host, tmp, &C.ord, &C.d_rs)) return -1;
    CkVecchiaModel& V = C.V;
    V.live = live_slots(h, free13);
    for (int b = 0; b < (h->n_procs == 1 ? 1 : 3); ++b)
        if (V.live >> ck_vg_nu_slot(h->n_procs, b) & 1u) V.nu_live |= 1u << b;
    if (lik_blocks(h, V.dnu)) return -1;
    V.blk5 = h->d_lik_blk;
    V.sig1 = h->par_sigma[0];
    V.sig2 = h->par_sigma[1];
    V.rho = h->par_rho;
    V.n_procs = h->n_procs;
    C.dvar = (V.live >> 11 & 3u) ? h->d_noise + Np : nullptr;
    HIPCHK(tmp.get(&C.d_gself, (size_t)N * sizeof(int)));
    HIPCHK(hipMemcpyAsync(C.d_gself, C.ord.gself.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, h->stream));
    // the select pass of every process (its points: the process's data in the caller's order)
    const int kl = ck_local_lds_limit();
    C.cnt2.assign((size_t)(2 * N), 0);
    int64_t n_over = 0;
    for (int k = 0; k < h->n_procs; ++k) {
        const int64_t m = h->n[k], soff = k == 0 ? 0 : n0;
        if (m == 0) continue;
        LocalPass& S = C.pass[k];
        if (local_pass(h, tmp, k, h->h_coords[k].data(), m, max_dist, 0, true, C.d_rs, C.ord.pos.data() + soff, nullptr, &S)) return -1;
        C.rep.st.add(S.st);
        for (int64_t p = 0; p < m; ++p) {
            const int k0 = S.sel[(size_t)(4 * p)], k1 = S.sel[(size_t)(4 * p + 1)], kt = k0 + k1;
            C.cnt2[(size_t)(2 * (soff + p))] = k0;
            C.cnt2[(size_t)(2 * (soff + p) + 1)] = k1;
            C.rep.n_empty += kt == 0;
            n_over += kt > kl;
            C.rep.k_max = std::max<int64_t>(C.rep.k_max, kt);
            C.n_pairs += (int64_t)(kt + 1) * (kt + 2) / 2;
            C.n_square += (int64_t)(kt + 1) * (kt + 1);
        }
    }
    if (n_over > 0) {
        write_select_timings(h, C.rep.st);   // the refused call's passes did run
        return fail(name + ": " + std::to_string(n_over) + " data have a conditioning set of more than " + std::to_string(kl) +
                    " data (the largest: " + std::to_string(C.rep.k_max) + "); " + refused_for);
    }
    return 0;
}

// Phase 2 of a gradient call, behind the stages: solve, back substitution and contraction, one workgroup per datum and one
// launch of k_vecchia_grad per process on the cut distances the select passes left on the device.  d_z (or null: the data):
// the values in the internal site order every read of the kernel sees -- the residual of ck_loglik_vecchia_trend_grad.  d_score:
// N x 13, the caller's stacked order.  D, mu, vv (all or none): what the terms need, the data gathered on the host while the
// device solves.  *solve_ms: the launches' device window ([ev2, ev3], read here).
static int vecchia_grad_solve(ck_handle* h, DevTemps& tmp, const VecchiaLdsStages& C, const double* d_z, double* d_score,
                              VecchiaData* D, std::vector<double>* mu, std::vector<double>* vv, double* solve_ms) {
    const int NP = CK_FISHER_NPAR;
    const int64_t n0 = h->n[0];
    CkVecchiaGradArgs A{};
    A.V = C.V;
    A.dvar = C.dvar;
    double *d_out[2] = {nullptr, nullptr}, *d_vv[2] = {nullptr, nullptr};
    for (int k = 0; k < h->n_procs; ++k) {
        const int64_t mp = C.pass[k].mp;   // this process's pass: the select in the stages, the solve here
        if (C.pass[k].m == 0) continue;
        HIPCHK(tmp.get(&d_out[k], (size_t)(2 * mp * 8)));
        HIPCHK(tmp.get(&d_vv[k], (size_t)(mp * 8)));
        HIPCHK(hipMemsetAsync(d_vv[k], 0, (size_t)(mp * 8), h->stream));
    }
    HIPCHK(hipEventRecord(h->ev2, h->stream));
    for (int k = 0; k < h->n_procs; ++k) {
        const LocalPass& S = C.pass[k];
        if (S.m == 0) continue;
        const int64_t soff = k == 0 ? 0 : n0;
        CkVecchiaGradArgs Ak = A;
        Ak.gself = C.d_gself + soff;
        Ak.score = d_score + soff * NP;
        CkLocalProblem P = S.prob;
        if (d_z) P.z = d_z;
        ck_launch_vecchia_grad(h->stream, P, S.m, S.d_cnt, d_out[k], d_out[k] + S.mp, d_vv[k], Ak);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(h->ev3, h->stream));
    if (D) {
        vecchia_data(h, D);   // on the host while the device solves: before the downloads, which wait for it
        for (int k = 0; k < h->n_procs; ++k) {
            const int64_t m = C.pass[k].m, soff = k == 0 ? 0 : n0;
            if (m == 0) continue;
            HIPCHK(hipMemcpyAsync(mu->data() + soff, d_out[k], m * 8, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipMemcpyAsync(vv->data() + soff, d_vv[k], m * 8, hipMemcpyDeviceToHost, h->stream));
        }
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(elapsed_ms(h->ev2, h->ev3, solve_ms));
    return 0;
}
// The column sums of the scores, in the caller's stacked order, and the scores themselves where asked for; first_bad != 0:
// grad13 is NaN.  *ms: the reduction's device window ([ev2, ev3], read here).
static int vecchia_score_sums(ck_handle* h, DevTemps& tmp, const double* d_score, int64_t first_bad, double* grad13,
                              double* score_host, double* ms) {
    const int NP = CK_FISHER_NPAR;
    const int64_t N = h->N, nblk = (N + 255) / 256;
    double *d_part = nullptr, *d_g = nullptr;
    HIPCHK(tmp.get(&d_part, (size_t)(nblk * NP) * 8));
    HIPCHK(tmp.get(&d_g, (size_t)NP * 8));
    HIPCHK(hipEventRecord(h->ev2, h->stream));
    ck_launch_vecchia_grad_sum(h->stream, N, d_score, d_part, d_g);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev3, h->stream));
    HIPCHK(hipMemcpyAsync(grad13, d_g, (size_t)NP * 8, hipMemcpyDeviceToHost, h->stream));
    if (score_host) HIPCHK(hipMemcpyAsync(score_host, d_score, (size_t)(N * NP) * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (first_bad)
        for (int k = 0; k < NP; ++k) grad13[k] = NAN;
    HIPCHK(elapsed_ms(h->ev2, h->ev3, ms));
    return 0;
}
// ck_timings [80 ..] of a gradient call (behind vecchia_report); reduce_ms: the terms' and the scores' reductions
static void vecchia_grad_timings(ck_handle* h, const VecchiaLdsStages& C, double reduce_ms) {
    h->t_ms[80] = C.rep.st.ms;
    h->t_ms[81] = C.rep.solve_ms;
    h->t_ms[82] = reduce_ms;
    h->t_ms[83] = C.rep.total_ms;
    h->t_ms[84] = (double)h->N;
    h->t_ms[85] = (double)C.n_pairs;
}

// The gradient of the Vecchia likelihood (include/cokrige.h has the definition, ck_vecchia_grad.h the formula).  Its own two
// phases instead of predict_local_impl's one: the stages above, then one launch of k_vecchia_grad per process on the cut
// distances the select passes left on the device, then the terms (vecchia_terms_tail: ck_loglik_vecchia's bits) and the column
// sums of the scores.
extern "C" int ck_loglik_vecchia_grad(ck_handle* h, const int64_t* rank_host, double max_dist, const int32_t* free13, double* out3,
                                      double* grad13, double* score_host, int64_t* stats3, int64_t* info) {
    CHKH(h);
    if (vecchia_admit(h, "ck_loglik_vecchia_grad", rank_host && out3 && grad13 ? nullptr : "rank_host / out3 / grad13", max_dist))
        return -1;
    const auto t_begin = std::chrono::steady_clock::now();
    timings_from(h, 72);
    const int NP = CK_FISHER_NPAR;
    for (int k = 0; k < NP; ++k) grad13[k] = NAN;
    const int64_t N = h->N, n0 = h->n[0];
    DevTemps tmp;
    VecchiaLdsStages C;
    if (vecchia_lds_stages(h, "ck_loglik_vecchia_grad",
                           "the gradient is for sets the LDS solver takes: lower the caps or the radius, or difference ck_loglik_vecchia",
                           rank_host, max_dist, free13, tmp, &C))
        return -1;
    VecchiaReport& rep = C.rep;
    double* d_score = nullptr;
    HIPCHK(tmp.get(&d_score, (size_t)(N * NP) * 8));
    std::vector<double> mu((size_t)N), vv((size_t)N, 0.0);
    VecchiaData D;
    if (vecchia_grad_solve(h, tmp, C, nullptr, d_score, &D, &mu, &vv, &rep.solve_ms)) return -1;
    int64_t first_bad = 0;
    if (vecchia_terms_tail(h, tmp, D, mu, vv, C.cnt2, out3, nullptr, nullptr, nullptr, &first_bad, &rep.n_lds, &rep.terms_ms)) return -1;
    double ms_sum = 0;
    if (vecchia_score_sums(h, tmp, d_score, first_bad, grad13, score_host, &ms_sum)) return -1;
    if (info) *info = first_bad;
    rep.total_ms = ms_since(t_begin);
    vecchia_report(h, rep, stats3);   // (n_tiled, grow_ms: 0 -- every set is of the LDS class)
    vecchia_grad_timings(h, C, rep.terms_ms + ms_sum);
    return 0;
}

// ---------------------------------------------------------------------------------------
// conditional simulation in the moving neighbourhood (include/cokrige.h has the definition)
// ---------------------------------------------------------------------------------------
// The search runs on an AUGMENTED data set: an internal handle on the caller's device and stream that holds the caller's model,
// metric, caps, noise and data, with the m sites appended to process i as noise-free pseudo-data of value 0.  Its precedence
// pointers put every datum in front of every site (rs = the datum's stacked index < N; a site: N + its position in the
// ordering), so local_pass on it is ck_loglik_vecchia's search on the augmented set.  The caller's handle is only read: no
// existing kernel changes and no call on it can lose its bits.  The internal handle lives as long as the call.
// The device memory a simulation call may still take: what the device reports, or option "sim_free_bytes" less what the call
// holds already (taken) -- the option stands for the whole device, the report shrinks by itself.
static int local_sim_free(const ck_handle* h, int64_t taken, size_t* fr) {
    size_t tot = 0;
    if (h->sim_free_bytes > 0)
        *fr = (size_t)std::max<int64_t>(0, h->sim_free_bytes - taken);
    else
        HIPCHK(hipMemGetInfo(fr, &tot));
    return 0;
}
struct HandleDeleter {
    void operator()(ck_handle* c) const { (void)ck_destroy(c); }
};
struct LocalSim {
    std::unique_ptr<ck_handle, HandleDeleter> child;
    int64_t N = 0, m = 0;    // m: the stacked sites of both processes
    int64_t mq[2] = {0, 0};
    std::vector<int> pos;    // the caller's stacked site index -> position in the ordering
    std::vector<int> ext;    // internal index of the augmented set -> the caller's stacked index (a site: N + its index)
    LocalPass pass;
    CkLocalSimOut out{};
    std::vector<int> ns, spos;
    std::vector<double> mu, s2;
    int64_t n_empty = 0, k_max = 0, w_bytes = 0;   // w_bytes: what the weight kernel's outputs hold on the device
    double weights_ms = 0.0;
};
// A launch's view of points [base, ..) of a pass as process i: the per-point arrays shifted, so that a kernel's point 0 is the
// pass's point `base`
static CkLocalProblem local_problem_from(const ck_handle* h, CkLocalProblem P, int64_t base, int i) {
    P.pc += base;   // (the three rows keep their stride mpad)
    P.pu += base;
    if (P.rq) P.rq += 2 * base;
    if (P.cp) P.cp += base;
    if (P.rp) P.rp += base;
    P.i_pred = i;
    P.c0var = h->blk[2 * i].amp + h->blk[2 * i].nugget;
    return P;
}
// What the entry points (name) do up to the weight kernel: the refusals, the ordering, the augmented set, the select pass (a
// set beyond the LDS limit is refused here, before any solve), then k_local_sim_weights and the downloads the host plans with.
// The sites: mq[q] of process q at pcs[q], stacked (ck_host.h: CkSimSites).  i: the process of ck_simulate_local, whose sites
// are the only ones; pair: the pair form, which needs a model of two processes (i is not read).
static int local_sim_stages(ck_handle* h, const std::string& name, int i, bool pair, const double* const pcs[2], const int64_t mq[2],
                            const int64_t* rank_host, double max_dist, const char* null_args, int64_t n_draws, DevTemps& tmp,
                            LocalSim* out) {
    LocalSim& C = *out;
    const int64_t m = mq[0] + mq[1];
    if (h->world != 1)
        return fail(name + " is the single-process form: this handle is partitioned (world = " + std::to_string(h->world) + ")");
    if (null_args) return fail(name + ": null " + null_args);
    if (m < 1) return fail(name + ": m = " + std::to_string(m) + " sites; at least 1");
    if (n_draws < 1) return fail(name + ": n_draws = " + std::to_string(n_draws) + "; at least 1");
    if (!(max_dist >= 0.0) || !std::isfinite(max_dist))
        return fail(name + ": max_dist must be finite and >= 0, got " + std::to_string(max_dist));
    if (trend_total(h) > 0)
        return fail(name + ": a trend of " + std::to_string(trend_total(h)) +
                    " columns is set on the handle; the local draws take none (clear it with ck_set_trend)");
    if (!h->model_set) return fail("ck_set_model has not been called");
    for (int k = 0; k < h->n_procs; ++k)
        if (!h->data_set[k]) return fail("ck_set_data missing for process " + std::to_string(k));
    if (!pair && (i < 0 || i >= h->n_procs)) return fail(name + ": process index out of range");
    if (pair && h->n_procs != 2) return fail(name + ": needs a model of two processes (n_procs = " + std::to_string(h->n_procs) + ")");
    const int64_t n0 = h->n[0];
    const int64_t N = C.N = n0 + (h->n_procs == 2 ? h->n[1] : 0);
    C.m = m;
    C.mq[0] = mq[0];
    C.mq[1] = mq[1];
    if (N <= 0) return fail("no observations");
    if (N + m > INT32_MAX) return fail(name + ": more than 2^31 - 1 data and sites");
    CkSimSites ST;   // ck_host.cpp: the ordering of the stacked sites, then their places in the augmented set
    if (ck_host_sim_order(rank_host, mq, &ST))
        return fail(name + ": sites " + std::to_string(ST.dup[0]) + " and " + std::to_string(ST.dup[1]) + " have the same rank " +
                    std::to_string((long long)rank_host[ST.dup[0]]));
    // ---- the augmented set
    {
        ck_handle* c = nullptr;
        if (ck_create(h->device, &c)) return -1;
        C.child.reset(c);
    }
    ck_handle* c = C.child.get();
    c->stream = h->stream;
    c->metric = h->metric;
    c->exact_cov = h->exact_cov;
    c->site_order = h->site_order;
    c->local_select_cap = h->local_select_cap;
    c->local_nmax[0] = h->local_nmax[0];
    c->local_nmax[1] = h->local_nmax[1];
    memcpy(c->blk, h->blk, sizeof(h->blk));
    c->n_procs = h->n_procs;
    c->par_sigma[0] = h->par_sigma[0];
    c->par_sigma[1] = h->par_sigma[1];
    c->par_rho = h->par_rho;
    HIPCHK(hipMemcpyAsync(c->d_blk, c->blk, 3 * sizeof(CkMatern), hipMemcpyHostToDevice, c->stream));
    c->model_set = true;
    for (int k = 0; k < h->n_procs; ++k) {
        std::vector<double> co(h->h_coords[k]), va(h->h_values[k]);
        if (mq[k] > 0) {
            co.insert(co.end(), pcs[k], pcs[k] + 2 * mq[k]);
            va.insert(va.end(), (size_t)mq[k], 0.0);
        }
        if (ck_set_data(c, k, co.data(), va.data(), (int64_t)va.size())) return -1;
        if (!h->noise_var[k].empty()) {
            std::vector<double> nv(h->noise_var[k]);
            nv.insert(nv.end(), (size_t)mq[k], 0.0);   // a site is a noise-free pseudo-datum
            if (ck_set_noise(c, k, nv.data(), (int64_t)nv.size(), h->noise_scale[k])) return -1;
        }
    }
    if (ensure_layout(c, false)) return -1;
    if (ensure_noise(c)) return -1;
    // ---- precedence: the data in front of every site, the sites by position
    ck_host_sim_ext(c->n_procs, h->n, mq, c->n0p, c->Npad, c->perm[0].data(), c->n_procs == 2 ? c->perm[1].data() : nullptr, &ST);
    C.pos = std::move(ST.pos);
    C.ext = std::move(ST.ext);
    int* d_rs = nullptr;
    HIPCHK(tmp.get(&d_rs, (size_t)c->Npad * sizeof(int)));
    HIPCHK(hipMemcpyAsync(d_rs, ST.rs.data(), (size_t)c->Npad * sizeof(int), hipMemcpyHostToDevice, c->stream));
    // ---- the select pass, once over the stacked sites (with cv = 0 the search does not look at the process); sets beyond the
    // LDS limit are refused before any solve
    std::vector<double> stacked;   // the pair form: both site sets behind each other
    const double* pts = mq[1] == 0 ? pcs[0] : pcs[1];
    if (mq[0] > 0 && mq[1] > 0) {
        stacked.assign(pcs[0], pcs[0] + 2 * mq[0]);
        stacked.insert(stacked.end(), pcs[1], pcs[1] + 2 * mq[1]);
        pts = stacked.data();
    }
    LocalPass& S = C.pass;
    if (local_pass(c, tmp, mq[0] > 0 ? 0 : 1, pts, m, max_dist, 0, true, d_rs, ST.rp.data(), nullptr, &S)) return -1;
    h->t_ms[110] = S.st.ms;
    const int kl = ck_local_lds_limit();
    int64_t n_over = 0;
    for (int64_t t = 0; t < m; ++t) {
        const int kt = S.cnt[(size_t)t];
        C.n_empty += kt == 0;
        n_over += kt > kl;
        C.k_max = std::max<int64_t>(C.k_max, kt);
    }
    if (n_over > 0)
        return fail(name + ": " + std::to_string(n_over) + " sites have a conditioning set of more than " + std::to_string(kl) +
                    " data (the largest: " + std::to_string(C.k_max) +
                    "); the draws are for sets the LDS solver takes: lower the caps or the radius");
    // ---- the weights
    const int64_t w_bytes = m * ((int64_t)kl * (2 * sizeof(int) + 2 * 8) + 2 * 8 + sizeof(int));
    {
        size_t fr = 0;
        if (local_sim_free(h, 0, &fr)) return -1;
        if ((size_t)w_bytes > fr)
            return fail(name + ": needs " + std::to_string(w_bytes) + " bytes of device memory for the weights of " + std::to_string(m) +
                        " sites; " + std::to_string(fr) + " bytes are available");
    }
    C.w_bytes = w_bytes;
    CkLocalSimOut& O = C.out;
    O.n_data = (int)N;
    HIPCHK(tmp.get(&O.gidx, (size_t)(m * kl) * sizeof(int)));
    HIPCHK(tmp.get(&O.spos, (size_t)(m * kl) * sizeof(int)));
    HIPCHK(tmp.get(&O.ns, (size_t)m * sizeof(int)));
    HIPCHK(tmp.get(&O.w, (size_t)(m * kl) * 8));
    HIPCHK(tmp.get(&O.sw, (size_t)(m * kl) * 8));
    HIPCHK(tmp.get(&O.mu, (size_t)m * 8));
    HIPCHK(tmp.get(&O.s2, (size_t)m * 8));
    HIPCHK(hipEventRecord(c->ev2, c->stream));
    for (int q = 0; q < 2; ++q) {   // one launch per process's sites: the kernel carries the process and its prior as uniforms
        if (mq[q] == 0) continue;
        const int64_t b = q == 0 ? 0 : mq[0];
        const CkLocalSimOut Oq{O.n_data, O.gidx + b * kl, O.spos + b * kl, O.ns + b, O.w + b * kl, O.sw + b * kl, O.mu + b, O.s2 + b};
        ck_launch_local_sim_weights(c->stream, local_problem_from(c, S.prob, b, q), mq[q], S.d_cnt + b, Oq);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev3, c->stream));
    C.ns.resize((size_t)m);
    C.spos.resize((size_t)(m * kl));
    C.mu.resize((size_t)m);
    C.s2.resize((size_t)m);
    HIPCHK(hipMemcpyAsync(C.ns.data(), O.ns, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(C.spos.data(), O.spos, (size_t)(m * kl) * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(C.mu.data(), O.mu, (size_t)m * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(C.s2.data(), O.s2, (size_t)m * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(elapsed_ms(c->ev2, c->ev3, &C.weights_ms));
    h->t_ms[111] = C.weights_ms;
    return 0;
}

// the weights of every stacked site behind local_sim_stages: members as stacked caller indices, ascending
static int local_sim_weights_out(ck_handle* h, const LocalSim& C, int64_t* idx_host, double* w_host) {
    const int64_t m = C.m;
    const int kl = ck_local_lds_limit();
    std::vector<int> gi((size_t)(m * kl));
    std::vector<double> w((size_t)(m * kl));
    HIPCHK(hipMemcpyAsync(gi.data(), C.out.gidx, gi.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(w.data(), C.out.w, w.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<std::pair<int64_t, double>> row;
    for (int64_t t = 0; t < m; ++t) {   // members as stacked caller indices, ascending
        row.clear();
        for (int a = 0; a < kl && gi[(size_t)(t * kl + a)] >= 0; ++a)
            row.push_back({(int64_t)C.ext[(size_t)gi[(size_t)(t * kl + a)]], w[(size_t)(t * kl + a)]});
        std::sort(row.begin(), row.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        for (int a = 0; a < kl; ++a) {
            idx_host[t * kl + a] = a < (int)row.size() ? row[(size_t)a].first : -1;
            w_host[t * kl + a] = a < (int)row.size() ? row[(size_t)a].second : 0.0;
        }
    }
    return 0;
}
// the sites of one process as the stacked sites of both
struct SimSites {
    const double* pcs[2] = {nullptr, nullptr};
    int64_t mq[2] = {0, 0};
    SimSites(int i, const double* pcoords, int64_t m) {
        pcs[i == 1 ? 1 : 0] = pcoords;
        mq[i == 1 ? 1 : 0] = m;
    }
    SimSites(const double* pc0, int64_t m0, const double* pc1, int64_t m1) {
        pcs[0] = pc0, pcs[1] = pc1;
        mq[0] = m0, mq[1] = m1;
    }
};
// the pair forms' own refusals, in front of local_sim_stages'
static int local_sim_pair_admit(const std::string& name, const SimSites& X) {
    if (X.mq[0] < 0 || X.mq[1] < 0)
        return fail(name + ": m0 = " + std::to_string(X.mq[0]) + ", m1 = " + std::to_string(X.mq[1]) + "; both must be >= 0");
    if ((X.mq[0] > 0 && !X.pcs[0]) || (X.mq[1] > 0 && !X.pcs[1])) return fail(name + ": null pcoords0_host / pcoords1_host");
    return 0;
}

extern "C" int ck_debug_simulate_local_weights(ck_handle* h, int i, const double* pcoords, int64_t m, const int64_t* rank_host,
                                               double max_dist, int64_t* idx_host, double* w_host) {
    CHKH(h);
    timings_from(h, 110);
    DevTemps tmp;
    LocalSim C;
    const SimSites X(i, pcoords, m);
    if (local_sim_stages(h, "ck_debug_simulate_local_weights", i, false, X.pcs, X.mq, rank_host, max_dist,
                         pcoords && rank_host && idx_host && w_host ? nullptr : "pcoords_host / rank_host / idx_host / w_host", 1, tmp, &C))
        return -1;
    return local_sim_weights_out(h, C, idx_host, w_host);
}

extern "C" int ck_debug_simulate_local_pair_weights(ck_handle* h, const double* pcoords0, int64_t m0, const double* pcoords1,
                                                    int64_t m1, const int64_t* rank_host, double max_dist, int64_t* idx_host,
                                                    double* w_host) {
    CHKH(h);
    const std::string name = "ck_debug_simulate_local_pair_weights";
    const SimSites X(pcoords0, m0, pcoords1, m1);
    if (local_sim_pair_admit(name, X)) return -1;
    timings_from(h, 110);
    DevTemps tmp;
    LocalSim C;
    if (local_sim_stages(h, name, 0, true, X.pcs, X.mq, rank_host, max_dist,
                         rank_host && idx_host && w_host ? nullptr : "rank_host / idx_host / w_host", 1, tmp, &C))
        return -1;
    return local_sim_weights_out(h, C, idx_host, w_host);
}

// Both simulation calls (name) behind their refusals: the stages above, the levels, the recursion chunk by chunk, the per-site
// outputs.  pair: count_host has four columns (the earlier sites split by process), else three.
static int simulate_local_impl(ck_handle* h, const std::string& name, int i, bool pair, const SimSites& X, const char* null_args,
                               const int64_t* rank_host, double max_dist, int64_t n_draws, uint64_t seed, const double* noise_host,
                               double* draws_host, double* mean_host, double* var_host, int32_t* count_host, int64_t* stats4,
                               int64_t* info) {
    const auto t_begin = std::chrono::steady_clock::now();
    timings_from(h, 110);
    DevTemps tmp;
    LocalSim C;
    if (local_sim_stages(h, name, i, pair, X.pcs, X.mq, rank_host, max_dist, null_args, n_draws, tmp, &C)) return -1;
    const int64_t m = C.m;
    const int kl = ck_local_lds_limit();
    // ---- the levels of the recursion
    const auto t_plan = std::chrono::steady_clock::now();
    CkSimLevels lv;
    const int64_t n_levels = ck_host_sim_levels(m, kl, C.pos.data(), C.ns.data(), C.spos.data(), &lv);
    if (n_levels < 0)
        return fail(name + ": site " + std::to_string(lv.off[0]) + " conditions on position " + std::to_string(lv.off[1]) +
                    ", which is not earlier than its own");
    h->t_ms[112] = ms_since(t_plan);
    int64_t first_bad = 0, n_site_nbr = 0;
    for (int64_t t = 0; t < m; ++t) {
        if (!first_bad && !(C.s2[(size_t)t] > 0.0)) first_bad = 1 + t;
        n_site_nbr += C.ns[(size_t)t];
    }
    // ---- the recursion, chunk by chunk
    const int64_t per_draw = m * 8 * 2;   // Y and the draws in the caller's order (the caller's noise is staged in the latter)
    int64_t chunk = h->draw_chunk;
    {
        size_t fr = 0;
        if (local_sim_free(h, C.w_bytes, &fr)) return -1;
        const int64_t need = 2 * per_draw + 2 * m * (int64_t)sizeof(int);
        if ((size_t)need > fr)
            return fail(name + ": needs " + std::to_string(need) + " bytes of device memory for a chunk of 2 draws at " +
                        std::to_string(m) + " sites; " + std::to_string(fr) + " bytes are available");
        if (chunk <= 0) chunk = std::min<int64_t>((int64_t)(fr / 2) / per_draw, 8192);
    }
    chunk = std::max<int64_t>(2, chunk & ~(int64_t)1);   // even: a thread makes the Box-Muller pair (d, d + 1)
    chunk = std::min<int64_t>(chunk, roundup(n_draws, 2));
    int *d_order = nullptr, *d_pos = nullptr;
    double *d_Y = nullptr, *d_X = nullptr;
    HIPCHK(tmp.get(&d_order, (size_t)m * sizeof(int)));
    HIPCHK(tmp.get(&d_pos, (size_t)m * sizeof(int)));
    HIPCHK(tmp.get(&d_Y, (size_t)(chunk * m) * 8));
    HIPCHK(tmp.get(&d_X, (size_t)(chunk * m) * 8));
    HIPCHK(hipMemcpyAsync(d_order, lv.order.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_pos, C.pos.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
    CkLocalSimLevel A{};
    A.pos = d_pos;
    A.ns = C.out.ns;
    A.spos = C.out.spos;
    A.sw = C.out.sw;
    A.mu = C.out.mu;
    A.s2 = C.out.s2;
    A.Y = d_Y;
    A.ldy = chunk;
    A.eps_in_y = noise_host ? 1 : 0;
    A.seed = seed;
    ck_handle* c = C.child.get();
    for (int64_t d0 = 0; d0 < n_draws; d0 += chunk) {
        const int64_t nd = std::min<int64_t>(chunk, n_draws - d0);
        A.d0 = d0;
        if (noise_host)   // staged where the chunk's draws will stand; the last chunk's download has ended (synchronised below)
            HIPCHK(hipMemcpyAsync(d_X, noise_host + d0 * m, (size_t)(nd * m) * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipEventRecord(c->ev0, h->stream));
        if (noise_host) ck_launch_local_sim_gather(h->stream, d_X, m, nd, d_pos, d_Y, chunk);
        for (int64_t l = 0; l < n_levels; ++l)   // one launch per level, in stream order: no waiting inside a kernel
            ck_launch_local_sim_level(h->stream, A, d_order + lv.off[(size_t)l], lv.off[(size_t)(l + 1)] - lv.off[(size_t)l]);
        ck_launch_local_sim_scatter(h->stream, d_Y, chunk, d_pos, m, nd, d_X);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->ev1, h->stream));
        HIPCHK(hipMemcpyAsync(draws_host + d0 * m, d_X, (size_t)(nd * m) * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        h->t_ms[113] += elapsed_ms(c->ev0, c->ev1);
    }
    // ---- the per-site outputs
    if (mean_host) memcpy(mean_host, C.mu.data(), (size_t)m * 8);
    if (var_host) memcpy(var_host, C.s2.data(), (size_t)m * 8);
    if (count_host) {
        std::vector<char> proc_at((size_t)m);   // by position: the process of the site there
        for (int64_t t = 0; t < m; ++t) proc_at[(size_t)C.pos[(size_t)t]] = t >= C.mq[0];
        for (int64_t t = 0; t < m; ++t) {
            int nsq[2] = {0, 0};   // the earlier sites of the set by process
            for (int a = 0; a < C.ns[(size_t)t]; ++a) ++nsq[(int)proc_at[(size_t)C.spos[(size_t)(t * kl + a)]]];
            const int d0n = C.pass.sel[(size_t)(4 * t)] - nsq[0], d1n = C.pass.sel[(size_t)(4 * t + 1)] - nsq[1];
            if (pair) {
                count_host[4 * t] = d0n;
                count_host[4 * t + 1] = d1n;
                count_host[4 * t + 2] = nsq[0];
                count_host[4 * t + 3] = nsq[1];
            } else {
                count_host[3 * t] = d0n;
                count_host[3 * t + 1] = d1n;
                count_host[3 * t + 2] = nsq[0] + nsq[1];
            }
        }
    }
    stats4[0] = C.n_empty;
    stats4[1] = C.k_max;
    stats4[2] = C.pass.st.n_capped;
    stats4[3] = n_levels;
    *info = first_bad;
    h->t_ms[114] = ms_since(t_begin);
    h->t_ms[115] = (double)(m - C.n_empty);
    h->t_ms[116] = (double)n_levels;
    h->t_ms[117] = (double)n_site_nbr;
    return 0;
}

extern "C" int ck_simulate_local(ck_handle* h, int i, const double* pcoords, int64_t m, const int64_t* rank_host, double max_dist,
                                 int64_t n_draws, uint64_t seed, const double* noise_host, double* draws_host, double* mean_host,
                                 double* var_host, int32_t* count_host, int64_t* stats4, int64_t* info) {
    CHKH(h);
    return simulate_local_impl(h, "ck_simulate_local", i, false, SimSites(i, pcoords, m),
                               pcoords && rank_host && draws_host && stats4 && info ? nullptr
                                                                                    : "pcoords_host / rank_host / draws_host / stats4 / info",
                               rank_host, max_dist, n_draws, seed, noise_host, draws_host, mean_host, var_host, count_host, stats4, info);
}

// Sequential Gaussian co-simulation: ck_simulate_local with the sites of both processes stacked behind the data (include/cokrige.h)
extern "C" int ck_simulate_local_pair(ck_handle* h, const double* pcoords0, int64_t m0, const double* pcoords1, int64_t m1,
                                      const int64_t* rank_host, double max_dist, int64_t n_draws, uint64_t seed,
                                      const double* noise_host, double* draws_host, double* mean_host, double* var_host,
                                      int32_t* count_host, int64_t* stats4, int64_t* info) {
    CHKH(h);
    const std::string name = "ck_simulate_local_pair";
    const SimSites X(pcoords0, m0, pcoords1, m1);
    if (local_sim_pair_admit(name, X)) return -1;
    return simulate_local_impl(h, name, 0, true, X, rank_host && draws_host && stats4 && info ? nullptr : "rank_host / draws_host / stats4 / info",
                               rank_host, max_dist, n_draws, seed, noise_host, draws_host, mean_host, var_host, count_host, stats4, info);
}

// ---------------------------------------------------------------------------------------
// the Vecchia likelihood with a GLS trend: profile ML and REML (include/cokrige.h has the definition, ck_vecchia_trend.h a
// datum's arithmetic)
// ---------------------------------------------------------------------------------------
// What the trend calls share behind vecchia_lds_stages.  vecchia_trend_solve: k_vecchia_trend on both processes, (mu, v . v,
// g = v . U) per datum in the caller's stacked order, on the device and on the host.  vecchia_trend_fit: the terms with their
// rows (vecchia_terms_tail), the Gram matrix G by its fixed tree, and on the host the GLS step on A = G[1:, 1:], b = G[1:, 0]
// (ck_predict_universal's: trend_gls_solve), out5 and the per-datum outputs.
#define CK_VT_REFUSED_FOR "the trend form is for sets the LDS solver takes: lower the caps or the radius"
struct VecchiaTrendFit {
    int p = 0;
    std::vector<double> mu, vv, g;   // N, N, N x p
    double* d_g = nullptr;
    std::vector<double> beta, cov;   // p, p x p (NaN with first_bad)
    double out5[5] = {NAN, NAN, NAN, NAN, NAN};
    int64_t first_bad = 0;
    double solve_ms = 0.0, gram_ms = 0.0;
};
static int vecchia_trend_solve(ck_handle* h, DevTemps& tmp, const VecchiaLdsStages& C, VecchiaTrendFit* F) {
    const int p = F->p = trend_total(h);
    const int64_t N = h->N, n0 = h->n[0];
    const size_t ng = (size_t)std::max<int64_t>(N * p, 1);
    double *d_mu = nullptr, *d_vv = nullptr;
    HIPCHK(tmp.get(&d_mu, (size_t)N * 8));
    HIPCHK(tmp.get(&d_vv, (size_t)N * 8));
    HIPCHK(tmp.get(&F->d_g, ng * 8));
    HIPCHK(hipMemsetAsync(d_mu, 0, (size_t)N * 8, h->stream));   // an empty set: no workgroup writes
    HIPCHK(hipMemsetAsync(d_vv, 0, (size_t)N * 8, h->stream));
    HIPCHK(hipMemsetAsync(F->d_g, 0, ng * 8, h->stream));
    const CkLocalTrend Tr{h->d_trendX, nullptr, h->trend_p[0], h->n_procs == 2 ? h->trend_p[1] : 0, CK_TREND_TOL};
    HIPCHK(hipEventRecord(h->ev2, h->stream));
    for (int k = 0; k < h->n_procs; ++k) {
        const LocalPass& S = C.pass[k];
        if (S.m == 0) continue;
        const int64_t soff = k == 0 ? 0 : n0;
        ck_launch_vecchia_trend(h->stream, S.prob, S.m, S.d_cnt, Tr, d_mu + soff, d_vv + soff, F->d_g + soff * p);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(h->ev3, h->stream));
    F->mu.resize((size_t)N);
    F->vv.resize((size_t)N);
    F->g.assign(ng, 0.0);
    HIPCHK(hipMemcpyAsync(F->mu.data(), d_mu, (size_t)N * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(F->vv.data(), d_vv, (size_t)N * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(F->g.data(), F->d_g, ng * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(elapsed_ms(h->ev2, h->ev3, &F->solve_ms));
    return 0;
}
static int vecchia_trend_fit(ck_handle* h, const char* name, int reml, DevTemps& tmp, VecchiaLdsStages& C, VecchiaTrendFit* F,
                             double* mean_host, double* var_host, int32_t* count_host) {
    if (vecchia_trend_solve(h, tmp, C, F)) return -1;
    const int p = F->p, NT = CK_VT_NTRI;
    const int64_t N = h->N, nblk = (N + 255) / 256;
    VecchiaData D;
    vecchia_data(h, &D);
    double *d_rows = nullptr, *d_part = nullptr, *d_tri = nullptr;
    HIPCHK(tmp.get(&d_rows, (size_t)(N * (p + 1)) * 8));
    HIPCHK(tmp.get(&d_part, (size_t)(nblk * NT) * 8));
    HIPCHK(tmp.get(&d_tri, (size_t)NT * 8));
    const CkVecchiaTrendRows T{p, h->Npad, h->d_trendX, C.d_gself, F->d_g, d_rows};
    double out3[3];
    if (vecchia_terms_tail(h, tmp, D, F->mu, F->vv, C.cnt2, out3, mean_host, var_host, count_host, &F->first_bad, &C.rep.n_lds,
                           &C.rep.terms_ms, &T))
        return -1;
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    ck_launch_vecchia_trend_gram(h->stream, N, p, d_rows, d_part, d_tri);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    double tri[CK_VT_NTRI] = {};
    HIPCHK(hipMemcpyAsync(tri, d_tri, (size_t)NT * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));   // (tri is stack memory)
    HIPCHK(elapsed_ms(h->ev0, h->ev1, &F->gram_ms));
    F->beta.assign((size_t)p, NAN);
    F->cov.assign((size_t)(p * p), NAN);
    if (F->first_bad == 0) {
        std::vector<double> A((size_t)(p * p)), b((size_t)p);
        for (int e = 0; e < (p + 1) * (p + 2) / 2; ++e) {
            int r, c;
            ck_vecchia_trend_pair(e, &r, &c);
            if (r > 0 && c == 0) b[(size_t)(r - 1)] = tri[e];
            if (c > 0) A[(size_t)((r - 1) * p + c - 1)] = A[(size_t)((c - 1) * p + r - 1)] = tri[e];
        }
        double logdet = 0.0;
        if (trend_gls_solve(h, name, p, A.data(), b.data(), nullptr, F->beta.data(), F->cov.data(), &logdet, nullptr)) return -1;
        const double q = ck_vecchia_trend_q(p, tri[0], b.data(), F->beta.data());
        F->out5[0] = ck_vecchia_trend_total(N, p, reml, out3[1], logdet, q);
        F->out5[1] = out3[1];
        F->out5[2] = logdet;
        F->out5[3] = q;
        F->out5[4] = tri[0];
    }
    if (mean_host) {   // mu_t + f_t . beta: the regressors of datum t in the columns of its process
        std::vector<double> x((size_t)p);
        for (int k = 0, col = 0; k < h->n_procs; col += h->trend_p[k], ++k) {
            const int pk = h->trend_p[k];
            const int64_t soff = k == 0 ? 0 : h->n[0];
            for (int64_t t = 0; t < h->n[k]; ++t) {
                std::fill(x.begin(), x.end(), 0.0);
                for (int c = 0; c < pk; ++c) x[(size_t)(col + c)] = h->trend_F[k][(size_t)(t * pk + c)];
                const int64_t s = soff + t;
                const int kt = C.cnt2[(size_t)(2 * s)] + C.cnt2[(size_t)(2 * s + 1)];
                mean_host[s] = ck_vecchia_trend_mean(mean_host[s], kt, p, x.data(), 1, F->g.data() + s * p, F->beta.data());
            }
        }
    }
    return 0;
}
static void vecchia_trend_out(const VecchiaTrendFit& F, double* out5, double* beta_host, double* beta_cov_host) {
    memcpy(out5, F.out5, sizeof(F.out5));
    if (beta_host) memcpy(beta_host, F.beta.data(), F.beta.size() * 8);
    if (beta_cov_host) memcpy(beta_cov_host, F.cov.data(), F.cov.size() * 8);
}
// ck_timings [96 ..] of a trend call (behind vecchia_report); grad_ms: the residual, k_vecchia_grad and the score sums
static void vecchia_trend_timings(ck_handle* h, const VecchiaLdsStages& C, const VecchiaTrendFit& F, double grad_ms) {
    h->t_ms[96] = C.rep.st.ms;
    h->t_ms[97] = F.solve_ms;
    h->t_ms[98] = C.rep.terms_ms + F.gram_ms;
    h->t_ms[99] = grad_ms;
    h->t_ms[100] = C.rep.total_ms;
    h->t_ms[101] = (double)h->N;
    h->t_ms[102] = (double)F.p;
}

extern "C" int ck_loglik_vecchia_trend(ck_handle* h, const int64_t* rank_host, double max_dist, int reml, double* out5,
                                       double* beta_host, double* beta_cov_host, double* mean_host, double* var_host,
                                       int32_t* count_host, int64_t* stats3, int64_t* info) {
    CHKH(h);
    const char* name = "ck_loglik_vecchia_trend";
    if (vecchia_admit(h, name, rank_host && out5 ? nullptr : "rank_host / out5", max_dist, true)) return -1;
    if (trend_total(h) == 0) {   // no trend: ck_loglik_vecchia, larger sets included
        double out3[3];
        if (vecchia_value(h, name, rank_host, max_dist, out3, mean_host, var_host, count_host, stats3, info)) return -1;
        const double o5[5] = {out3[0], out3[1], out3[0] == out3[0] ? 0.0 : NAN, out3[2], out3[2]};
        memcpy(out5, o5, sizeof(o5));
        return 0;
    }
    const auto t_begin = std::chrono::steady_clock::now();
    timings_from(h, 72);
    DevTemps tmp;
    VecchiaLdsStages C;
    if (vecchia_lds_stages(h, name, CK_VT_REFUSED_FOR, rank_host, max_dist, nullptr, tmp, &C)) return -1;
    VecchiaTrendFit F;
    if (vecchia_trend_fit(h, name, reml != 0, tmp, C, &F, mean_host, var_host, count_host)) return -1;
    vecchia_trend_out(F, out5, beta_host, beta_cov_host);
    if (info) *info = F.first_bad;
    C.rep.solve_ms = F.solve_ms;
    C.rep.total_ms = ms_since(t_begin);
    vecchia_report(h, C.rep, stats3);   // (n_tiled, grow_ms: 0 -- every set is of the LDS class)
    vecchia_trend_timings(h, C, F, 0.0);
    return 0;
}

// The gradient of the profiled value at beta = beta-hat (the envelope theorem): the stages of the value call, then
// k_vecchia_residual and ck_loglik_vecchia_grad's phase 2 and score sums on the residual.
extern "C" int ck_loglik_vecchia_trend_grad(ck_handle* h, const int64_t* rank_host, double max_dist, const int32_t* free13,
                                            double* out5, double* beta_host, double* beta_cov_host, double* grad13,
                                            double* score_host, int64_t* stats3, int64_t* info) {
    CHKH(h);
    const char* name = "ck_loglik_vecchia_trend_grad";
    if (vecchia_admit(h, name, rank_host && out5 && grad13 ? nullptr : "rank_host / out5 / grad13", max_dist, true)) return -1;
    if (trend_total(h) == 0) {   // no trend: ck_loglik_vecchia_grad
        double out3[3];
        if (ck_loglik_vecchia_grad(h, rank_host, max_dist, free13, out3, grad13, score_host, stats3, info)) return -1;
        const double o5[5] = {out3[0], out3[1], out3[0] == out3[0] ? 0.0 : NAN, out3[2], out3[2]};
        memcpy(out5, o5, sizeof(o5));
        return 0;
    }
    const auto t_begin = std::chrono::steady_clock::now();
    timings_from(h, 72);
    const int NP = CK_FISHER_NPAR;
    for (int k = 0; k < NP; ++k) grad13[k] = NAN;
    const int64_t N = h->N;
    DevTemps tmp;
    VecchiaLdsStages C;
    if (vecchia_lds_stages(h, name, CK_VT_REFUSED_FOR, rank_host, max_dist, free13, tmp, &C)) return -1;
    VecchiaTrendFit F;
    if (vecchia_trend_fit(h, name, 0, tmp, C, &F, nullptr, nullptr, nullptr)) return -1;
    vecchia_trend_out(F, out5, beta_host, beta_cov_host);
    if (info) *info = F.first_bad;
    double grad_ms = 0.0;
    if (F.first_bad) {   // no beta-hat, so no residual: every score is NaN
        if (score_host)
            for (int64_t e = 0; e < N * NP; ++e) score_host[e] = NAN;
    } else {
        double *d_res = nullptr, *d_score = nullptr;
        HIPCHK(tmp.get(&d_res, (size_t)h->Npad * 8));
        HIPCHK(tmp.get(&d_score, (size_t)(N * NP) * 8));
        CkVecchiaTrendBeta B{};
        for (int j = 0; j < F.p; ++j) B.b[j] = F.beta[(size_t)j];
        ck_launch_vecchia_residual(h->stream, h->Npad, F.p, h->z, h->d_trendX, B, d_res);
        HIPCHK(hipGetLastError());
        double ms_solve = 0.0, ms_sum = 0.0;
        if (vecchia_grad_solve(h, tmp, C, d_res, d_score, nullptr, nullptr, nullptr, &ms_solve)) return -1;
        if (vecchia_score_sums(h, tmp, d_score, 0, grad13, score_host, &ms_sum)) return -1;
        grad_ms = ms_solve + ms_sum;
    }
    C.rep.solve_ms = F.solve_ms;
    C.rep.total_ms = ms_since(t_begin);
    vecchia_report(h, C.rep, stats3);   // (n_tiled, grow_ms: 0 -- every set is of the LDS class)
    vecchia_trend_timings(h, C, F, grad_ms);
    return 0;
}

// the per-datum solve of the trend calls alone (the test surface of k_vecchia_trend): mu = v . y, v . v and g = v . U (N x p)
// in the caller's stacked order, zeros where the set is empty
extern "C" int ck_debug_vecchia_trend(ck_handle* h, const int64_t* rank_host, double max_dist, double* mu_host, double* vv_host,
                                      double* g_host) {
    CHKH(h);
    const char* name = "ck_debug_vecchia_trend";
    if (vecchia_admit(h, name, rank_host && mu_host && vv_host && g_host ? nullptr : "rank_host / mu_host / vv_host / g_host",
                      max_dist, true))
        return -1;
    timings_from(h, 72);
    DevTemps tmp;
    VecchiaLdsStages C;
    if (vecchia_lds_stages(h, name, CK_VT_REFUSED_FOR, rank_host, max_dist, nullptr, tmp, &C)) return -1;
    VecchiaTrendFit F;
    if (vecchia_trend_solve(h, tmp, C, &F)) return -1;
    memcpy(mu_host, F.mu.data(), (size_t)h->N * 8);
    memcpy(vv_host, F.vv.data(), (size_t)h->N * 8);
    memcpy(g_host, F.g.data(), (size_t)(h->N * F.p) * 8);
    write_select_timings(h, C.rep.st);
    return 0;
}

// The expected information of the Vecchia likelihood (include/cokrige.h has the definition, ck_vecchia_info.h the formula): the
// stages of the gradient call, one launch of k_vecchia_info per process, the fixed tree over the workgroups' 91-vectors, and on
// the host the mirror to 13 x 13.  No terms are formed: the result does not depend on the values.
extern "C" int ck_loglik_vecchia_fisher(ck_handle* h, const int64_t* rank_host, double max_dist, const int32_t* free13,
                                        double* fisher_host, int64_t* stats3, int64_t* info) {
    CHKH(h);
    if (vecchia_admit(h, "ck_loglik_vecchia_fisher", rank_host && fisher_host ? nullptr : "rank_host / fisher_host", max_dist))
        return -1;
    const auto t_begin = std::chrono::steady_clock::now();
    timings_from(h, 72);
    const int NP = CK_FISHER_NPAR, NT = CK_VI_NTRI;
    for (int k = 0; k < NP * NP; ++k) fisher_host[k] = NAN;
    const int64_t N = h->N, n0 = h->n[0];
    DevTemps tmp;
    VecchiaLdsStages C;
    if (vecchia_lds_stages(h, "ck_loglik_vecchia_fisher", "the information is for sets the LDS solver takes: lower the caps or the radius",
                           rank_host, max_dist, free13, tmp, &C))
        return -1;
    // one row of 91 partial sums per workgroup: a fixed run of consecutive data of a process, whatever the device
    const int64_t run = ck_vecchia_info_run();
    const int64_t rows0 = (n0 + run - 1) / run, rows1 = h->n_procs == 2 ? (h->n[1] + run - 1) / run : 0, n_rows = rows0 + rows1;
    const int64_t nblk = (n_rows + 255) / 256;
    double *d_rows = nullptr, *d_part = nullptr, *d_tri = nullptr;
    long long* d_bad = nullptr;
    HIPCHK(tmp.get(&d_rows, (size_t)(std::max<int64_t>(n_rows, 1) * NT) * 8));
    HIPCHK(tmp.get(&d_part, (size_t)(std::max<int64_t>(nblk, 1) * NT) * 8));
    HIPCHK(tmp.get(&d_tri, (size_t)NT * 8));
    HIPCHK(tmp.get(&d_bad, (size_t)std::max<int64_t>(n_rows, 1) * sizeof(long long)));
    HIPCHK(hipEventRecord(h->ev2, h->stream));
    for (int k = 0; k < h->n_procs; ++k) {
        const LocalPass& S = C.pass[k];
        if (S.m == 0) continue;
        const int64_t soff = k == 0 ? 0 : n0;
        CkVecchiaInfoArgs A{};
        A.V = C.V;
        A.dvar = C.dvar;
        A.gself = C.d_gself + soff;
        A.part = d_rows;
        A.bad = d_bad;
        A.row0 = k == 0 ? 0 : rows0;
        A.stacked0 = soff;
        ck_launch_vecchia_info(h->stream, S.prob, S.m, S.d_cnt, A);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(h->ev3, h->stream));
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    ck_launch_vecchia_info_sum(h->stream, n_rows, d_rows, d_part, d_tri);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    double tri[CK_VI_NTRI] = {};
    std::vector<long long> bad((size_t)n_rows, 0);
    if (n_rows > 0) {
        HIPCHK(hipMemcpyAsync(tri, d_tri, (size_t)NT * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(bad.data(), d_bad, (size_t)n_rows * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));   // (tri is stack memory)
    int64_t first_bad = 0;   // the rows come in the stacked order of their data
    for (int64_t r = 0; r < n_rows && first_bad == 0; ++r) first_bad = bad[(size_t)r];
    ck_vecchia_info_mirror(tri, C.V.live, first_bad != 0, fisher_host);
    if (info) *info = first_bad;
    double ms_sum = 0.0;
    VecchiaReport& rep = C.rep;
    if (n_rows > 0) {
        HIPCHK(elapsed_ms(h->ev2, h->ev3, &rep.solve_ms));
        HIPCHK(elapsed_ms(h->ev0, h->ev1, &ms_sum));
    }
    rep.n_lds = N;
    rep.total_ms = ms_since(t_begin);
    vecchia_report(h, rep, stats3);   // (terms_ms, n_tiled, grow_ms: 0 -- no terms, every set is of the LDS class)
    h->t_ms[88] = rep.st.ms;
    h->t_ms[89] = rep.solve_ms;
    h->t_ms[90] = ms_sum;
    h->t_ms[91] = rep.total_ms;
    h->t_ms[92] = (double)N;
    h->t_ms[93] = (double)C.n_square;
    return 0;
}

// The reference builds the local predictor's state once, in its constructor (src/point_prediction.py:24-43: the full Sigma
// blocks); here that state is the scratch slab of the large-neighbourhood paths.  nbytes > 0: at least that much; 0: the
// automatic budget of ck_predict_local (a quarter of the free memory, at most 32 GiB; option "local_slab_mb" if set).  After
// this call no ck_predict_local whose batches fit pays a hipMalloc.
extern "C" int ck_local_reserve(ck_handle* h, int64_t nbytes) {
    CHKH(h);
    if (nbytes < 0) return fail("ck_local_reserve: negative size");
    long long want = nbytes / 8;
    if (nbytes == 0 && local_budget_doubles(h, &want)) return -1;
    if (want <= local_slab_doubles(h)) return 0;
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(h->local_slab.reserve((size_t)want));
    h->t_ms[14] = ms_since(t0);
    return 0;
}

// ---------------------------------------------------------------------------------------
// empirical (cross-)variogram: src/fields.py:192-232
// ---------------------------------------------------------------------------------------
// Upload one field's points.  From 2 048 points on (and unless site_order = 0) they are first laid out along a
// Hilbert curve: bins sums and counts do not depend on the order of the points (up to rounding of the sums), and
// compact blocks of points are what lets the kernels skip whole pair tiles (ck_vario.hip, "tile culling").
// host_coords / host_vals receive the points in the order the device sees them (pairs come back as indices).
static int vario_upload(ck_handle* h, const double* coords, const double* vals, int64_t n, DevBuf<double>& u, DevBuf<double>& v,
                        std::vector<double>& host_coords, std::vector<double>& host_vals) {
    host_coords.assign(coords, coords + 2 * n);
    host_vals.assign(vals, vals + n);
    if (h->site_order && n >= 2048) {
        double lo[2] = {1e300, 1e300}, hi[2] = {-1e300, -1e300};
        ck_host_bounding_box(coords, n, lo, hi);
        std::vector<int64_t> perm;
        ck_host_hilbert_order(coords, n, lo, hi, perm);
        ck_host_parallel(n, [&](int, int64_t b, int64_t e2) {
            for (int64_t k = b; k < e2; ++k) {
                const int64_t e = perm[(size_t)k];
                host_coords[2 * k] = coords[2 * e];
                host_coords[2 * k + 1] = coords[2 * e + 1];
                host_vals[(size_t)k] = vals[e];
            }
        });
    }
    DevTemps tmp;
    double* stage = nullptr;
    HIPCHK(u.reserve((size_t)(3 * n)));
    HIPCHK(v.reserve((size_t)n));
    HIPCHK(tmp.get(&stage, (size_t)(2 * n * 8)));
    HIPCHK(hipMemcpyAsync(stage, host_coords.data(), 2 * n * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(v, host_vals.data(), n * 8, hipMemcpyHostToDevice, h->stream));
    ck_launch_vario_prep(h->stream, stage, n, h->metric, u, u + n, u + 2 * n);
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int ck_vario_begin(ck_handle* h, const double* coords_i, const double* resid_i, int64_t n_i,
                              const double* coords_j, const double* resid_j, int64_t n_j, int same) {
    CHKH(h);
    if (n_i <= 0 || !coords_i || !resid_i) return fail("bad field i");
    if (!same && (n_j <= 0 || !coords_j || !resid_j)) return fail("bad field j");
    // the binning kernel addresses the "j" arrays with 32-bit byte offsets (8 n_j < 2^32) and lists pairs as int indices
    if (n_i >= (1LL << 28) || n_j >= (1LL << 28)) return fail("at most 2^28 - 1 points per field");
    h->vg = {};
    h->vg_same = same ? 1 : 0;
    h->vg_ni = n_i;
    if (vario_upload(h, coords_i, resid_i, n_i, h->vg.iu, h->vg.iv, h->vg_ci, h->vg_vi)) return -1;
    if (same) {
        h->vg_nj = n_i;
        h->vg_cj = h->vg_ci;
        h->vg_vj = h->vg_vi;
        h->vg.ju = h->vg.iu;
        h->vg.jv = h->vg.iv;
    } else {
        h->vg_nj = n_j;
        if (vario_upload(h, coords_j, resid_j, n_j, h->vg.ju_own, h->vg.jv_own, h->vg_cj, h->vg_vj)) return -1;
        h->vg.ju = h->vg.ju_own;
        h->vg.jv = h->vg.jv_own;
    }
    HIPCHK(h->vg.ib64.reserve((size_t)(4 * ck_vario_nblocks(h->vg_ni, 64))));
    HIPCHK(h->vg.jb.reserve((size_t)(4 * ck_vario_nblocks(h->vg_nj, CK_VG_JCHUNK))));
    HIPCHK(h->vg.jbsub.reserve((size_t)(4 * ck_vario_nblocks(h->vg_nj, CK_VG_JSUB))));
    HIPCHK(h->vg.best.reserve(2));
    ck_launch_vario_bounds(h->stream, h->vg.iu, h->vg_ni, 64, h->vg.ib64);
    ck_launch_vario_bounds(h->stream, h->vg.ju, h->vg_nj, CK_VG_JCHUNK, h->vg.jb);
    ck_launch_vario_bounds(h->stream, h->vg.ju, h->vg_nj, CK_VG_JSUB, h->vg.jbsub);
    HIPCHK(hipGetLastError());
    h->vg_bgrid = ck_vario_bin_grid(h->vg_ni, h->vg_nj);
    HIPCHK(h->vg.part.reserve((size_t)h->vg_bgrid));
    HIPCHK(h->vg.psum.reserve((size_t)h->vg_bgrid * CK_VG_MAXBINS));
    HIPCHK(h->vg.pcnt.reserve((size_t)h->vg_bgrid * (CK_VG_MAXBINS + 1)));
    static_assert(CK_VG_ARGS_BYTES % 8 == 0, "vg.out is counted in 8-byte words");
    HIPCHK(h->vg.out.reserve(3 * (CK_VG_MAXBINS + 2) + CK_VG_MAXBINS + CK_VG_MAXBINS + 1 + CK_VG_ARGS_BYTES / 8));
    HIPCHK(h->vg.count.reserve(1));
    HIPCHK(h->vg.list.reserve((size_t)1 << 20));
    for (int k = 0; k < 4; ++k) h->vg_stats[k] = 0;
    return 0;
}

// the list a kernel has just filled, on the host; *overflow = the kernel wanted more room than the list has --
// the list is then re-allocated and the caller runs the kernel again
static int vario_fetch_list(ck_handle* h, std::vector<CkVarioPair>& out, bool* overflow) {
    unsigned cnt = 0;
    HIPCHK(hipMemcpyAsync(&cnt, h->vg.count, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *overflow = cnt > (unsigned)h->vg.list.cap();
    if (*overflow) {
        h->vg.list.reset();
        const uint64_t want = (uint64_t)cnt + cnt / 4 + 1024;
        if (want > 0xfffffff0ull) return fail("variogram: too many pairs on a bin edge for the host list");
        HIPCHK(h->vg.list.reserve((size_t)want));
        return 0;
    }
    out.resize(cnt);
    if (cnt) HIPCHK(hipMemcpy(out.data(), h->vg.list, (size_t)cnt * sizeof(CkVarioPair), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int ck_vario_extent(ck_handle* h, double max_dist, double* lo, double* hi, int64_t* n_positive) {
    CHKH(h);
    if (!h->vg.iu) return fail("ck_vario_begin has not been called");
    if (!(max_dist >= 0.0)) return fail("max_dist must be >= 0");
    *lo = *hi = NAN;
    *n_positive = 0;
    const int metric = h->metric;
    const double qcap0 = ck_host_vario_q_of_dist(metric, max_dist);
    double cap = qcap0 + ck_host_vario_band(metric, qcap0);   // pairs up to here may still have d <= max_dist
    bool have_lo = false, have_hi = false;
    double best_lo = INFINITY, best_hi = -1.0;
    // Round 0 normally settles both extremes.  Further rounds only when every pair within the band of the largest
    // q <= cap turns out to lie beyond max_dist: the cap then moves below them.
    // best_lo / best_hi over the candidates of one list, by the reference's own arithmetic (ck_host.cpp)
    auto decide = [&](const std::vector<CkVarioPair>& cand) {
        ck_host_vario_decide_extent(metric, h->vg_ci.data(), h->vg_cj.data(), cand.data(), (int64_t)cand.size(), max_dist,
                                    &best_lo, &best_hi);
        have_hi = best_hi >= 0.0;
        have_lo = best_lo < INFINITY;
    };
    for (int round = 0; round < 64 && !have_hi; ++round) {
        // The pass lists, on its way, every pair in a thin window under the cap: with dense data the largest retained q
        // lies inside it, and the candidates for the largest distance are then complete without a second pass.
        const double win = fmax(1e-9 * cap, 8.0 * ck_host_vario_band(metric, cap));
        const double qwin_lo = cap - win;
        HIPCHK(hipMemsetAsync(h->vg.count, 0, sizeof(unsigned), h->stream));
        ck_launch_vario_extent(h->stream, h->vg_bgrid, h->vg_same, h->vg.iu, h->vg_ni, h->vg.ju, h->vg_nj, cap, h->vg.part,
                               h->rank, h->world, h->vg.ib64, h->vg.jb, h->vg.jbsub, ck_host_vario_cmax(cap), h->vg.best, qwin_lo,
                               h->vg.list, h->vg.count, (unsigned)h->vg.list.cap());
        HIPCHK(hipGetLastError());
        std::vector<CkVarioExt> part(h->vg_bgrid);
        HIPCHK(hipMemcpyAsync(part.data(), h->vg.part, h->vg_bgrid * sizeof(CkVarioExt), hipMemcpyDeviceToHost, h->stream));
        std::vector<CkVarioPair> wcand;
        bool woverflow = false;
        if (vario_fetch_list(h, wcand, &woverflow)) return -1;   // synchronises the stream
        CkVarioExt best = part[0];
        for (int g = 1; g < h->vg_bgrid; ++g) {
            if (part[g].rmin < best.rmin) {
                best.rmin = part[g].rmin;
                best.imin = part[g].imin;
            }
            if (part[g].rmax > best.rmax) {
                best.rmax = part[g].rmax;
                best.imax = part[g].imax;
            }
        }
        if (best.imax < 0) break;   // no pair with q <= cap at all
        // every pair whose q is within the band of an extreme is a candidate; the reference's formula decides
        double qtop_lo = best.rmax - 2.0 * ck_host_vario_band(metric, best.rmax);
        const double qbot_hi = (!have_lo && best.imin >= 0) ? best.rmin + 2.0 * ck_host_vario_band(metric, best.rmin) : -1.0;
        bool top_done = false;
        if (!woverflow && qtop_lo >= qwin_lo) {   // the window holds every top candidate
            h->vg_stats[0] += (int64_t)wcand.size();
            decide(wcand);
            top_done = have_hi;   // else: all of them beyond max_dist -> the full candidate pass below, then a lower cap
        }
        if (!top_done || qbot_hi > 0.0) {
            std::vector<CkVarioPair> cand;
            const double top_from = top_done ? INFINITY : qtop_lo;   // top candidates already decided: the bottom ones only
            for (int pass = 0; pass < 3; ++pass) {
                HIPCHK(hipMemsetAsync(h->vg.count, 0, sizeof(unsigned), h->stream));
                ck_launch_vario_collect(h->stream, h->vg_bgrid, h->vg_same, h->vg.iu, h->vg_ni, h->vg.ju, h->vg_nj, top_from, cap,
                                        qbot_hi, h->vg.list, h->vg.count, (unsigned)h->vg.list.cap(), h->rank, h->world, h->vg.ib64, h->vg.jb,
                                        h->vg.jbsub);
                HIPCHK(hipGetLastError());
                bool overflow = false;
                if (vario_fetch_list(h, cand, &overflow)) return -1;
                if (!overflow) break;
                if (pass == 2) return fail("variogram: candidate list kept overflowing");
            }
            h->vg_stats[0] += (int64_t)cand.size();
            decide(cand);
        }
        if (round) h->vg_stats[3] += 1;
        if (!have_hi) {
            if (!(qtop_lo > 0.0)) break;
            cap = nextafter(qtop_lo, 0.0);   // everything from qtop_lo up is beyond max_dist
        }
    }
    if (have_hi) *hi = best_hi;
    if (have_lo) *lo = best_lo;
    *n_positive = (have_lo && have_hi) ? 1 : 0;
    return 0;
}

extern "C" int ck_vario_bin(ck_handle* h, double max_dist, const double* edges, int n_edges, int covariogram,
                            double* sums, int64_t* counts) {
    CHKH(h);
    if (!h->vg.iu) return fail("ck_vario_begin has not been called");
    const int nb = n_edges - 1;
    if (nb < 1 || nb > CK_VG_MAXBINS) return fail("n_bins must be between 1 and " + std::to_string(CK_VG_MAXBINS));
    for (int b = 0; b < nb; ++b)
        if (!(edges[b + 1] > edges[b])) return fail("bin edges must increase");
    if (edges[0] != 0.0) return fail("first bin edge must be 0 (src/fields.py:402)");
    if (!(max_dist > 0.0)) return fail("max_dist must be positive");
    const int metric = h->metric;
    // levels, their rounding bands and the clusters of levels whose bands overlap: ck_host.cpp
    CkVarioLevels lv;
    if (ck_host_vario_levels(metric, max_dist, edges, nb, &lv)) return -1;
    const int E = lv.E, EC = lv.EC;
    const double *cxa = lv.cxa, *cxb = lv.cxb, *cthr = lv.cthr;
    const int* clast = lv.clast;
    const double q_reach = lv.q_reach;
    double* d_xa = h->vg.out;
    double* d_xb = h->vg.out + (CK_VG_MAXBINS + 2);
    double* d_dthr = h->vg.out + 2 * (CK_VG_MAXBINS + 2);
    double* d_sums = h->vg.out + 3 * (CK_VG_MAXBINS + 2);
    long long* d_cnt = (long long*)(d_sums + CK_VG_MAXBINS);
    void* d_args = (void*)(d_cnt + CK_VG_MAXBINS + 1);
    HIPCHK(hipMemcpyAsync(d_xa, cxa, (EC + 1) * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_xb, cxb, (EC + 1) * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d_dthr, cthr, (EC + 1) * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));   // the arrays are on the stack
    std::vector<CkVarioPair> fix;
    for (int pass = 0; pass < 3; ++pass) {
        HIPCHK(hipMemsetAsync(h->vg.count, 0, sizeof(unsigned), h->stream));
        HIPCHK(hipEventRecord(h->ev0, h->stream));
        ck_launch_vario_bin(h->stream, metric, h->vg_same, covariogram ? 1 : 0, h->vg.iu, h->vg.iv, h->vg_ni, h->vg.ju,
                            h->vg.jv, h->vg_nj, EC, d_xa, d_xb, d_dthr, ck_host_vario_cmax(q_reach), h->vg.ib64, h->vg.jb, h->vg.jbsub,
                            h->vg_bgrid, h->vg.psum, h->vg.pcnt, h->vg.list, h->vg.count, (unsigned)h->vg.list.cap(), h->rank, h->world,
                            EC, d_sums, d_cnt, d_args);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->ev1, h->stream));
        bool overflow = false;
        if (vario_fetch_list(h, fix, &overflow)) return -1;
        if (!overflow) break;
        if (pass == 2) return fail("variogram: edge-pair list kept overflowing");
    }
    long long dcn[CK_VG_MAXBINS + 1], cnt[CK_VG_MAXBINS + 1];
    std::vector<double> dsm(CK_VG_MAXBINS, 0.0), sm(CK_VG_MAXBINS + 1, 0.0);
    HIPCHK(hipMemcpyAsync(dsm.data(), d_sums, EC * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(dcn, d_cnt, (CK_VG_MAXBINS + 1) * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int b = 0; b <= CK_VG_MAXBINS; ++b) cnt[b] = 0;
    for (int k = 0; k < EC; ++k) {   // device bin k -> real bin clast[k] (< E: bins from the cap up hold nothing)
        sm[(size_t)clast[k]] = dsm[(size_t)k];
        cnt[clast[k]] = dcn[k];
    }
    // The pairs inside the band of a level (cluster) were binned below it; the reference's formula on libm decides.
    ck_host_vario_fix(metric, h->vg_ci.data(), h->vg_cj.data(), h->vg_vi.data(), h->vg_vj.data(), fix.data(), (int64_t)fix.size(),
                      lv, covariogram ? 1 : 0, sm.data(), cnt);
    for (int b = E; b < nb; ++b) {   // bins above the cap hold nothing
        sm[(size_t)b] = 0.0;
        cnt[b] = 0;
    }
    for (int b = 0; b < nb; ++b) {
        sums[b] = sm[(size_t)b];
        counts[b] = cnt[b];
    }
    h->vg_stats[1] = (int64_t)fix.size();
    h->vg_stats[2] = dcn[CK_VG_MAXBINS];
    HIPCHK(elapsed_ms(h->ev0, h->ev1, &h->t_ms[9]));
    return 0;
}

extern "C" int ck_vario_stats(ck_handle* h, int64_t* out, int n) {
    CHKH(h);
    for (int k = 0; k < n && k < 4; ++k) out[k] = h->vg_stats[k];
    return 0;
}

extern "C" int ck_vario_end(ck_handle* h) {
    CHKH(h);
    h->vg = {};
    return 0;
}

// ---------------------------------------------------------------------------------------
// diagnostics
// ---------------------------------------------------------------------------------------
// ck_matern_grad per lag on the device, with the stencil blocks and the step lik_blocks hands the likelihood kernels
extern "C" int ck_debug_matern_grad(ck_handle* h, int block, const double* lags, int64_t n, double* out3) {
    CHKH(h);
    if (!h->model_set) return fail("ck_set_model has not been called");
    if (block < 0 || block >= (h->n_procs == 1 ? 1 : 3)) return fail("ck_debug_matern_grad: block index out of range");
    if (n <= 0) return 0;
    if (!lags || !out3) return fail("ck_debug_matern_grad: null array");
    double dnu3[3] = {0.0, 0.0, 0.0};
    if (lik_blocks(h, dnu3)) return -1;
    DevTemps tmp;
    double *dl = nullptr, *dO = nullptr;
    HIPCHK(tmp.get(&dl, (size_t)(n * 8)));
    HIPCHK(tmp.get(&dO, (size_t)(3 * n * 8)));
    HIPCHK(hipMemcpyAsync(dl, lags, n * 8, hipMemcpyHostToDevice, h->stream));
    ck_launch_debug_matern_grad(h->stream, h->d_lik_blk + 5 * block, dnu3[block], dl, n, dO);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out3, dO, 3 * n * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int ck_debug_site_order(ck_handle* h, int k, int64_t* perm_out, int64_t n_k) {
    CHKH(h);
    if (k < 0 || k >= h->n_procs) return fail("process index out of range");
    if (ensure_layout(h)) return -1;
    if (n_k != h->n[k]) return fail("n_k must equal the number of observations of process k");
    for (int64_t j = 0; j < n_k; ++j) perm_out[j] = h->perm[k][(size_t)j];
    return 0;
}

extern "C" int ck_debug_get_lower(ck_handle* h, double* out, int64_t n) {
    CHKH(h);
    if (!h->assembled) return fail("nothing assembled");
    if (n != h->N) return fail("n must equal the number of observations");
    memset(out, 0, (size_t)n * n * 8);
    const int64_t gap = h->n0p - h->n[0];
    auto ext = [&](int64_t g) -> int64_t {   // internal 0-based -> external 0-based, -1 for padding
        if (g < h->n[0]) return g;
        if (g >= h->n0p && g < h->nend) return g - gap;
        return -1;
    };
    return read_lower(h, h->sig, h->nK, h->Npad, [&](int64_t R, int64_t C, double v) {
        const int64_t er = ext(R), ec = ext(C);
        if (er >= 0 && ec >= 0) out[er * n + ec] = v;
    });
}

// out[e] = entry (rows[e], cols[e]) of the lower triangle held in the packed panels (internal, padded indices; r >= c)
__global__ void k_gather_entries(double* const* __restrict__ sigptr, const long long* __restrict__ rows,
                                 const long long* __restrict__ cols, long n, double* __restrict__ out) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const long r = rows[e], c = cols[e];
    const long K = c / CK_NB;
    out[e] = sigptr[K][(r - K * CK_NB) * CK_NB + (c - K * CK_NB)];
}

extern "C" int ck_debug_get_entries(ck_handle* h, const int64_t* rows, const int64_t* cols, int64_t n, double* out) {
    CHKH(h);
    if (!h->assembled) return fail("ck_assemble_joint has not been called");
    if (h->world != 1) return fail("ck_debug_get_entries is the single-process form");
    if (n < 0 || (n > 0 && (!rows || !cols || !out))) return fail("bad arguments");
    if (n == 0) return 0;
    // caller's stacked index (process 0 sites, then process 1) -> internal padded index
    std::vector<int64_t> inv((size_t)h->N);
    for (int k = 0; k < h->n_procs; ++k) {
        const int64_t off_c = k == 0 ? 0 : h->n[0], off_i = k == 0 ? 0 : h->n0p;
        for (int64_t j = 0; j < h->n[k]; ++j) inv[(size_t)(off_c + h->perm[k][(size_t)j])] = off_i + j;
    }
    std::vector<long long> hr((size_t)n), hc((size_t)n);
    for (int64_t e = 0; e < n; ++e) {
        if (rows[e] < 0 || rows[e] >= h->N || cols[e] < 0 || cols[e] >= h->N) return fail("entry index out of range");
        long long r = inv[(size_t)rows[e]], c = inv[(size_t)cols[e]];
        if (r < c) std::swap(r, c);   // symmetric: only the lower triangle is stored
        hr[(size_t)e] = r;
        hc[(size_t)e] = c;
    }
    DevTemps tmp;
    long long *dr = nullptr, *dc = nullptr;
    double* dout = nullptr;
    HIPCHK(tmp.get(&dr, (size_t)n * 8));
    HIPCHK(tmp.get(&dc, (size_t)n * 8));
    HIPCHK(tmp.get(&dout, (size_t)n * 8));
    HIPCHK(hipMemcpyAsync(dr, hr.data(), (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(dc, hc.data(), (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    k_gather_entries<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream>>>(h->d_sigptr, dr, dc, (long)n, dout);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// Phase profile of the 64 x 64 diagonal-block kernel on a well-conditioned block: out[0..5] = microseconds of
// load | factorisation | scaling + store | inverse of the diagonal 16 x 16 blocks | off-diagonal blocks | store of the
// inverse (shader clock / 100 MHz reference), out[6] = the whole kernel by HIP events, out[7] = the same for the product
// kernel (k_potrf64), average over `iters` back-to-back launches.
extern "C" int ck_debug_potrf_profile(ck_handle* h, int iters, double* out8) {
    CHKH(h);
    if (!out8 || iters < 1) return fail("bad arguments");
    DevTemps tmp;
    double *dA = nullptr, *dL = nullptr;
    long long *dprof = nullptr, *dinfo = nullptr;
    HIPCHK(tmp.get(&dA, 64 * 512 * 8));
    HIPCHK(tmp.get(&dL, 64 * 64 * 8));
    HIPCHK(tmp.get(&dprof, 16 * 8));
    HIPCHK(tmp.get(&dinfo, 8));
    std::vector<double> A((size_t)64 * 512, 0.0);
    for (int i = 0; i < 64; ++i)
        for (int j = 0; j <= i; ++j) A[(size_t)i * 512 + j] = (i == j ? 70.0 : 0.0) + 1.0 / (1.0 + i + j);
    HIPCHK(hipMemsetAsync(dinfo, 0, 8, h->stream));
    HIPCHK(hipMemsetAsync(dprof, 0, 16 * 8, h->stream));
    double clk_mhz = 100.0;   // provisional unit; rescaled below so that the phases add up to the instrumented launch
    long long hp[16];
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int it = 0; it < 4; ++it) {
        HIPCHK(hipMemcpyAsync(dA, A.data(), A.size() * 8, hipMemcpyHostToDevice, h->stream));
        ck_launch_potrf64_prof(h->stream, dA, 512, dinfo, dL, dprof);
        HIPCHK(hipMemcpyAsync(hp, dprof, sizeof(hp), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (it)
            for (int k = 0; k < 6; ++k) acc[k] += (double)(hp[k + 1] - hp[k]) / clk_mhz / 3.0;
    }
    for (int k = 0; k < 6; ++k) out8[k] = acc[k];
    for (int which = 0; which < 2; ++which) {
        HIPCHK(hipMemcpyAsync(dA, A.data(), A.size() * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipEventRecord(h->ev0, h->stream));
        for (int it = 0; it < iters; ++it) {   // refactoring the factor is harmless for timing (it stays positive definite enough)
            if (which == 0)
                ck_launch_potrf64_prof(h->stream, dA, 512, dinfo, dL, dprof);
            else
                ck_launch_potrf64(h->stream, dA, 512, 0, dinfo, dL);
        }
        HIPCHK(hipEventRecord(h->ev1, h->stream));
        HIPCHK(hipEventSynchronize(h->ev1));
        double ms = 0;
        HIPCHK(elapsed_ms(h->ev0, h->ev1, &ms));
        out8[6 + which] = ms * 1e3 / iters;
    }
    {   // s_memtime ticks at the shader clock: scale the phases so that they add up to the instrumented launch's duration
        double sum = 0;
        for (int k = 0; k < 6; ++k) sum += out8[k];
        if (sum > 0)
            for (int k = 0; k < 6; ++k) out8[k] *= out8[6] / sum;
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// Where a link of the cooperative panel step's chain spends its time: k_panel_coop on a well-conditioned rows x 512 panel;
// out[8 * b + k], b = 1 .. 7: microseconds from the moment chunk b saw the pivot chunk's "rows final" flag (k = 0) to
// k = 1 accumulation done | 2 inverse flag seen | 3 rows solved and stored | 4 drained + rows flag set | 5 diagonal block
// updated | 6 factored + inverse stored | 7 drained + flag set; out[0] = the whole launch by HIP events, out[1] = shader MHz.
extern "C" int ck_debug_coop_profile(ck_handle* h, int64_t rows, double* out64) {
    CHKH(h);
    if (!out64 || rows < CK_NB || rows % 64) return fail("bad arguments");
    DevTemps tmp;
    double *dP = nullptr;
    long long *dprof = nullptr, *dinfo = nullptr;
    HIPCHK(tmp.get(&dP, (size_t)panel_payload(rows, 0)));
    HIPCHK(tmp.get(&dprof, 64 * 8));
    HIPCHK(tmp.get(&dinfo, 8));
    std::vector<double> A((size_t)rows * CK_NB);
    for (int64_t i = 0; i < rows; ++i)
        for (int j = 0; j < CK_NB; ++j) A[(size_t)i * CK_NB + j] = (i == j ? 600.0 : 0.0) + 1.0 / (1.0 + (double)(i % 977) + j);
    long long hp[64];
    double ms = 0;
    for (int it = 0; it < 3; ++it) {
        HIPCHK(hipMemcpyAsync(dP, A.data(), A.size() * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemsetAsync(dinfo, 0, 8, h->stream));
        HIPCHK(hipMemsetAsync(dprof, 0, 64 * 8, h->stream));
        h->coop_seq += 1;
        HIPCHK(hipEventRecord(h->ev0, h->stream));
        ck_launch_panel_coop_prof(h->stream, dP, rows, dP + rows * CK_NB, 0, dinfo, h->d_coop, h->coop_seq, h->d_coop + 16, dprof);
        HIPCHK(hipEventRecord(h->ev1, h->stream));
        HIPCHK(hipMemcpyAsync(hp, dprof, sizeof(hp), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(elapsed_ms(h->ev0, h->ev1, &ms));
    }
    HIPCHK(hipGetLastError());
    // the chain from link 1's first stamp to link 7's last takes (launch - head - tail); the stamps tick at the shader clock:
    // calibrate it on the span of the whole chain against the event time is too coarse -- report ticks / 2 400 MHz
    const double mhz = 2400.0;
    for (int k = 0; k < 64; ++k) out64[k] = 0.0;
    for (int b = 1; b <= 7; ++b)
        for (int k = 1; k < 8; ++k) out64[8 * b + k] = (double)(hp[8 * b + k] - hp[8 * b]) / mhz;
    for (int b = 2; b <= 7; ++b) out64[8 * b] = (double)(hp[8 * b] - hp[8 * (b - 1)]) / mhz;   // link-to-link period
    out64[0] = ms * 1e3;
    out64[1] = mhz;
    return 0;
}

// Diagnostic: do small dependent kernels on the high-priority side stream run WHILE a chip-filling trailing update is being
// dispatched on the main stream, or only after its grid has been placed?  (What a look-ahead of the panel chain under
// the bulk of the previous group's update needs.)  On an assembled, unfactored handle of >= 8 panels (Sigma is destroyed:
// assemble again afterwards): mode 0: the update alone | 1: n_side cooperative panel steps on a scratch panel of `rows`
// rows alone | 2: both -- the first side kernel submitted in front of the update and released by the same event, the others
// behind it in stream order.  out[0] = update ms (mode 1: 0), out[1 + i] = end of side kernel i after the common start, ms.
extern "C" int ck_debug_stream_overlap(ck_handle* h, int mode, int64_t rows, int n_side, double* out) {
    CHKH(h);
    if (!h->assembled || h->factored || h->nK < 8 || h->world != 1) return fail("needs an assembled, unfactored single-process handle of >= 8 panels");
    if (!out || rows < CK_NB || rows % 64 || n_side < 0 || n_side > 16 || mode < 0 || mode > 2) return fail("bad arguments");
    HIPCHK(hipSetDevice(h->device));
    DevTemps tmp;
    double* dP = nullptr;
    long long* dinfo = nullptr;
    HIPCHK(tmp.get(&dP, (size_t)panel_payload(rows, 0)));
    HIPCHK(tmp.get(&dinfo, 8));
    std::vector<double> A((size_t)rows * CK_NB);
    for (int64_t i = 0; i < rows; ++i)
        for (int j = 0; j < CK_NB; ++j) A[(size_t)i * CK_NB + j] = (i == j ? 600.0 : 0.0) + 1.0 / (1.0 + (double)(i % 977) + j);
    HIPCHK(hipMemcpyAsync(dP, A.data(), A.size() * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(dinfo, 0, 8, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    struct Events {   // destroyed on every return path (the HIPCHK early returns used to leak them)
        std::vector<hipEvent_t> v;
        ~Events() {
            for (hipEvent_t e : v)
                if (e) (void)hipEventDestroy(e);
        }
    } evs;
    evs.v.assign((size_t)n_side + 2, nullptr);
    std::vector<hipEvent_t>& ev = evs.v;
    for (auto& e : ev) HIPCHK(hipEventCreate(&e));
    hipStream_t M = h->stream, S = h->side;
    HIPCHK(hipEventRecord(ev[0], M));
    if (mode >= 1) {
        HIPCHK(hipStreamWaitEvent(S, ev[0], 0));
        for (int i = 0; i < n_side; ++i) {
            h->coop_seq += 1;
            ck_launch_panel_coop(S, dP, rows, dP + rows * CK_NB, 0, dinfo, h->d_coop, h->coop_seq, h->d_coop + 16);
            HIPCHK(hipEventRecord(ev[2 + i], S));
        }
    }
    if (mode != 1) sigma_update_on(h, M, 0, 3, 3, 1, h->nK - 3, false);
    HIPCHK(hipEventRecord(ev[1], M));
    HIPCHK(hipStreamSynchronize(M));
    HIPCHK(hipStreamSynchronize(S));
    HIPCHK(hipGetLastError());
    double ms = 0;
    HIPCHK(elapsed_ms(ev[0], ev[1], &ms));
    out[0] = mode != 1 ? ms : 0.0;
    for (int i = 0; i < n_side; ++i) {
        out[1 + i] = 0.0;
        if (mode >= 1) {
            HIPCHK(elapsed_ms(ev[0], ev[2 + i], &ms));
            out[1 + i] = ms;
        }
    }
    h->assembled = false;
    return 0;
}

extern "C" int ck_debug_mfma_probe(ck_handle* h, int32_t* out) {
    CHKH(h);
    DevBuf<int32_t> d;
    HIPCHK(d.reserve(64 * 4 * 3));
    ck_launch_mfma_probe(h->stream, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d, 64 * 4 * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int ck_estimate_bytes(ck_handle* h, int64_t m, int64_t* out) {
    CHKH(h);
    for (int k = 0; k < h->n_procs; ++k)
        if (!h->data_set[k]) return fail("ck_set_data missing for process " + std::to_string(k));
    const int64_t n1 = h->n_procs == 2 ? h->n[1] : 0;
    const int64_t Np = roundup((n1 > 0 ? roundup(h->n[0], 64) : h->n[0]) + n1, CK_NB);
    const int nK = (int)(Np / CK_NB);
    // what dev_alloc is asked for by ensure_layout, build_panels and aux_begin_impl, each request rounded as it rounds
    auto al = align256;
    int64_t tot = 2 * al(site_bytes(Np)) + al(value_bytes(Np));
    for (int K = h->rank; K < nK; K += h->world) tot += panel_bytes(Np, K);
    tot += 2 * al(ptr_bytes(nK));
    if (h->world > 1) tot += (int64_t)h->recv_slots * al(recv_bytes(Np));
    const int64_t mpad = roundup(m + 1, CK_AUX_ALIGN);
    tot += al(rhs_bytes(mpad, Np)) + 2 * al(site_bytes(mpad)) + 2 * al(pair_bytes(mpad));
    *out = tot + 4096;
    return 0;
}

extern "C" int ck_debug_cu_probe(ck_handle* h, const uint32_t* cu_mask8, int n_wg, uint32_t* out) {
    CHKH(h);
    if (n_wg <= 0 || n_wg > 65536 || !out) return fail("bad n_wg");
    hipStream_t st = nullptr;
    if (cu_mask8)
        HIPCHK(hipExtStreamCreateWithCUMask(&st, 8, cu_mask8));
    else
        HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    DevBuf<unsigned> d;
    HIPCHK(d.reserve((size_t)n_wg));
    HIPCHK(hipMemsetAsync(d, 0xff, (size_t)n_wg * 4, st));
    ck_launch_cu_probe(st, d, n_wg, 4);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d, (size_t)n_wg * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    (void)hipStreamDestroy(st);
    return 0;
}

extern "C" int ck_debug_mfma_peak(ck_handle* h, int waves_per_simd, int iters, double* out3) {
    CHKH(h);
    if (waves_per_simd < 1 || waves_per_simd > 8 || iters < 1) return fail("bad arguments");
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, h->device));
    const int cus = prop.multiProcessorCount;
    DevBuf<double> sink;
    HIPCHK(sink.reserve(4));
    const int threads = 256, blocks = cus * waves_per_simd;   // 4 waves per block = one per SIMD
    ck_launch_mfma_peak(h->stream, blocks, waves_per_simd, 10, sink);   // warm-up
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    const int nacc = ck_launch_mfma_peak(h->stream, blocks, waves_per_simd, iters, sink);
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipEventSynchronize(h->ev1));
    HIPCHK(hipGetLastError());
    double ms = 0;
    HIPCHK(elapsed_ms(h->ev0, h->ev1, &ms));
    const double flops = (double)blocks * (threads / 64) * (double)iters * nacc * 2048.0;
    double hs[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpy(hs, sink, 32, hipMemcpyDeviceToHost));
    out3[0] = flops / (ms * 1e-3) / 1e12;                           // TFLOP/s
    out3[1] = hs[2] > 0 ? hs[1] / hs[2] * 100.0 : 0.0;              // in-kernel shader clock, MHz
    out3[2] = hs[1] / ((double)iters * nacc);   // cycles per MFMA of one wave
    return 0;
}

// Diagnostic: the clock the chip holds under the trailing-update kernel on the data of the last factorisation.  With
// option "gemm_stamps" = 1 every workgroup of k_syrk_group_d leaves the shader cycles and 100 MHz ticks of its
// lifetime; out6 = median / 5 % / 95 % quantile of the shader clock in MHz over the stamped workgroups, their number,
// the median lifetime in shader cycles and in microseconds.
extern "C" int ck_debug_gemm_clock(ck_handle* h, double* out6) {
    CHKH(h);
    if (!h->d_stamps) return fail("ck_debug_gemm_clock: set option gemm_stamps = 1 and factor first");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<unsigned long long> st(4 * h->n_stamps);
    HIPCHK(hipMemcpy(st.data(), h->d_stamps, st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::vector<double> mhz, cyc;
    for (size_t b = 0; b < h->n_stamps; ++b)
        if (st[4 * b + 1] > 1000) {   // > 10 us: a workgroup that ran a tile
            mhz.push_back((double)st[4 * b] / (double)st[4 * b + 1] * 100.0);
            cyc.push_back((double)st[4 * b]);
        }
    for (int i = 0; i < 6; ++i) out6[i] = 0;
    if (mhz.empty()) return 0;
    std::sort(mhz.begin(), mhz.end());
    std::sort(cyc.begin(), cyc.end());
    out6[0] = mhz[mhz.size() / 2];
    out6[1] = mhz[mhz.size() / 20];
    out6[2] = mhz[mhz.size() - 1 - mhz.size() / 20];
    out6[3] = (double)mhz.size();
    out6[4] = cyc[cyc.size() / 2];
    out6[5] = out6[4] / out6[0];
    return 0;
}

// raw stamps of the last stamped launch: out[4 b .. 4 b + 3] = shader cycles, 100 MHz ticks of workgroup b's lifetime (0, 0
// if it returned at once), its start in 100 MHz ticks, XCC_ID << 32 | HW_ID; grid4 = grid x, y, first block column, panels
extern "C" int ck_debug_gemm_stamps(ck_handle* h, uint64_t* out_host, int64_t n_words, int64_t* grid4) {
    CHKH(h);
    if (!h->d_stamps) return fail("ck_debug_gemm_stamps: set option gemm_stamps and factor first");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t n = std::min<size_t>((size_t)std::max<int64_t>(n_words, 0), 4 * h->n_stamps);
    HIPCHK(hipMemcpy(out_host, h->d_stamps, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) grid4[i] = h->stamp_grid[i];
    return 0;
}

extern "C" int ck_set_option(ck_handle* h, const char* name, int64_t value) {
    CHKH(h);
    if (!name) return fail("null option name");
    if (!strcmp(name, "gemm_stamps")) {   // diagnostic, see ck_debug_gemm_clock; after the first assemble
        h->d_stamps.reset();
        h->n_stamps = 0;
        if (value != 0) {
            if (!h->layout_ready) return fail("gemm_stamps: assemble first");
            HIPCHK(hipSetDevice(h->device));
            const size_t n = (size_t)(h->Npad / 128) * (CK_NB / 128) * (size_t)(h->Npad / CK_NB);
            HIPCHK(h->d_stamps.reserve(4 * n));
            h->n_stamps = n;
            HIPCHK(hipMemset(h->d_stamps, 0, 4 * h->n_stamps * sizeof(unsigned long long)));
        }
        h->stamp_sel = (int)value;
        return 0;
    }
    if (!strcmp(name, "time_gemm")) {
        if (value < 0 || value > 2) return fail("time_gemm must be 0, 1 or 2");
        h->time_gemm = (int)value;
        return 0;
    }
    if (!strcmp(name, "fused_sweeps")) {
        if (value < -1 || value > 1) return fail("fused_sweeps must be -1 (automatic), 0 or 1");
        h->fused_sweeps_opt = (int)value;
        return 0;
    }
    if (!strcmp(name, "fused_prio")) {   // see ck_handle::fused_prio
        if (value < 0 || value > 2) return fail("fused_prio must be 0, 1 or 2");
        h->fused_prio = (int)value;
        return 0;
    }
    if (!strcmp(name, "coop_spins")) {
        if (value < 1000 || value > 2000000000LL) return fail("coop_spins must be in [1000, 2e9]");
        h->coop_spins = (unsigned)value;
        return 0;
    }
    if (!strcmp(name, "coop_inject_panel")) {   // tests: the bounded wait of k_panel_coop must trip and be recovered from
        if (value < -1) return fail("coop_inject_panel must be -1 (off) or a panel index");
        h->coop_inject_panel = (int)value;
        return 0;
    }
    if (!strcmp(name, "group_first") || !strcmp(name, "group_tail") || !strcmp(name, "group_tail_panels")) {   // see group_plan()
        if (value < (strcmp(name, "group_first") ? 0 : -1) || value > 1024) return fail("group_first (-1 = automatic) / group_tail / group_tail_panels must be in [0, 1024]");
        (!strcmp(name, "group_first") ? h->group_first : !strcmp(name, "group_tail") ? h->group_tail : h->group_tail_panels) = (int)value;
        return 0;
    }
    if (!strcmp(name, "assemble_queue")) {   // see ck_handle::assemble_queue
        if (value < -1 || value > 4096) return fail("assemble_queue must be in [-1, 4096]");
        h->assemble_queue = (int)value;
        return 0;
    }
    if (!strcmp(name, "local_left")) {   // see ck_handle::local_left
        if (value < 0 || value > 1) return fail("local_left must be 0 or 1");
        h->local_left = (int)value;
        return 0;
    }
    if (!strcmp(name, "tall_split")) {
        if (value < 0 || value > 2) return fail("tall_split must be 0, 1 or 2");
        h->tall_split = (int)value;
        return 0;
    }
    if (!strcmp(name, "solve_la")) {
        if (value < -1 || value > 1) return fail("solve_la must be -1, 0 or 1");
        h->solve_la = (int)value;
        return 0;
    }
    if (!strcmp(name, "tall_b2_stream")) {
        h->tall_b2_stream = value != 0;
        return 0;
    }
    if (!strcmp(name, "tall_thin")) {
        if (value < 0 || value > 1) return fail("tall_thin must be 0 or 1");
        h->tall_thin = (int)value;
        return 0;
    }
    if (!strcmp(name, "tall_split_rows")) {
        if (value < 0) return fail("tall_split_rows must be >= 0");
        h->tall_split_rows = (int)std::min<int64_t>(value, 1 << 30);
        return 0;
    }
    if (!strcmp(name, "tall_sweep")) {   // see ck_handle::tall_sweep
        if (value < 0 || value > 1) return fail("tall_sweep must be 0 or 1");
        h->tall_sweep = (int)value;
        return 0;
    }
    if (!strcmp(name, "fused_la")) {
        if (value < -1 || value > 1) return fail("fused_la must be -1 (automatic), 0 or 1");
        h->fused_la = (int)value;
        return 0;
    }
    if (!strcmp(name, "fused_group")) {
        if (value < 0 || value > 16) return fail("fused_group must be in [0, 16]");
        h->fused_group = (int)value;
        return 0;
    }
    if (!strcmp(name, "lookahead")) {   // see ck_handle::lookahead
        if (value < -1 || value > 1) return fail("lookahead must be -1 (automatic), 0 or 1");
        h->lookahead = (int)value;
        return 0;
    }
    if (!strcmp(name, "local_slab_mb")) {
        if (value < 0) return fail("local_slab_mb must be >= 0");
        h->local_slab_mb = value;
        return 0;
    }
    if (!strcmp(name, "panel_fused")) {   // see ck_handle::panel_fused
        if (value < 0 || value > 31) return fail("panel_fused must be in [0, 31]");
        h->panel_fused = (int)value;
        return 0;
    }
    if (!strcmp(name, "local_group")) {
        if (value < 1 || value > CK_LT_NINV) return fail("local_group must be in [1, 8]");
        h->local_group = (int)value;
        return 0;
    }
    if (!strcmp(name, "local_select_cap")) {   // see ck_handle::local_select_cap (tests: the re-scan path at small sizes)
        if (value < 1 || value > ck_local_select_capacity())
            return fail("local_select_cap must be in [1, " + std::to_string(ck_local_select_capacity()) + "]");
        h->local_select_cap = (int)value;
        return 0;
    }
    if (!strcmp(name, "local_tile_min")) {   // see ck_handle::local_tile_min
        if (value < 0) return fail("local_tile_min must be >= 0");
        h->local_tile_min = (int)std::min<int64_t>(value, 1 << 30);
        return 0;
    }
    if (!strcmp(name, "panel_group")) {   // panels per trailing update (1 = after every panel)
        if (value < 0 || value > 16) return fail("panel_group must be in [0, 16] (0 = automatic)");
        h->panel_group = (int)value;
        return 0;
    }
    if (!strcmp(name, "site_order")) {   // 0: caller's order | 1: Hilbert order (see ck_handle::site_order)
        if (h->layout_ready && (value != 0) != (h->site_order != 0)) {
            // same sizes, other order: the sites are laid out again on the next assemble (what ck_factor does on its own
            // to report a failing minor in the caller's numbering; the step-wise driver does it through this option)
            h->layout_ready = false;
            h->assembled = h->factored = false;
            h->aux_state = AUX_NONE;
        }
        h->site_order = value != 0;
        return 0;
    }
    if (!strcmp(name, "recv_slots")) {   // see ck_handle::recv_slots; before the first assemble / ck_estimate_bytes
        if (value < 2 || value > 64) return fail("recv_slots must be in [2, 64]");
        if (h->layout_ready || !h->sig.empty()) return fail("recv_slots must be set before the panels are allocated");
        h->recv_slots = (int)value;
        return 0;
    }
    if (!strcmp(name, "block_chunk")) {   // ck_predict_blocks: prediction sites per K2 assembly (0 = automatic)
        if (value < 0) return fail("block_chunk must be >= 0 (0 = automatic)");
        h->block_chunk = value;
        return 0;
    }
    if (!strcmp(name, "fisher_product_mb")) {   // ck_loglik_fisher: MiB the stored products may take (0 = automatic)
        if (value < 0) return fail("fisher_product_mb must be >= 0 (0 = automatic)");
        h->fisher_product_mb = value;
        return 0;
    }
    if (!strcmp(name, "sim_free_bytes")) {   // ck_simulate_local: the bytes that count as free (0 = what the device reports)
        if (value < 0) return fail("sim_free_bytes must be >= 0 (0 = automatic)");
        h->sim_free_bytes = value;
        return 0;
    }
    if (!strcmp(name, "draw_chunk")) {   // ck_conditional_draws: draws per product launch (0 = automatic)
        if (value < 0) return fail("draw_chunk must be >= 0 (0 = automatic)");
        h->draw_chunk = value;
        return 0;
    }
    if (!strcmp(name, "exact_cov")) {   // 1: per-entry Bessel evaluation instead of the tables
        h->exact_cov = value != 0;
        return 0;
    }
    return fail(std::string("unknown option ") + name);
}

extern "C" int ck_table_info(ck_handle* h, int block, int* enabled, int* n_intervals, double* q_lo, double* q_hi,
                             double* max_rel_err) {
    CHKH(h);
    if (block < 0 || block > 2) return fail("block must be 0 (11), 1 (12) or 2 (22)");
    if (ensure_layout(h)) return -1;
    const CkTable& T = h->tab[block];
    if (enabled) *enabled = T.enabled;
    if (n_intervals) *n_intervals = T.n_int;
    if (q_lo) *q_lo = T.q_lo;
    if (q_hi) *q_hi = T.q_hi;
    if (max_rel_err) *max_rel_err = T.max_rel_err;
    return 0;
}

extern "C" int ck_table_fallbacks(ck_handle* h, int reset, int64_t* count) {
    CHKH(h);
    if (count) *count = h->fallback_total;
    if (reset) h->fallback_total = 0;
    return 0;
}

extern "C" int ck_timings(ck_handle* h, double* out, int n) {
    CHKH(h);
    for (int k = 0; k < n && k < CK_N_TIMINGS; ++k) out[k] = h->t_ms[k];
    return 0;
}

extern "C" int ck_dev_gemm_nt(ck_handle* h, double* C, int64_t ldc, const double* A, int64_t lda, const double* B,
                              int64_t ldb, int64_t M, int64_t N, int64_t K, int lower) {
    CHKH(h);
    if (M % CK_BM || N % 64 || K % 16) return fail("ck_dev_gemm_nt: M % 256, N % 64, K % 16 must be 0");
    ck_launch_gemm_nt(h->stream, C, ldc, A, lda, B, ldb, M, N, K, lower, 0, 1, 0, 0, 0);
    HIPCHK(hipGetLastError());
    return 0;
}
