// ck_la.hip -- dense FP64 linear algebra kernels for gfx950 (MI355X), all on v_mfma_f64_16x16x4_f64.
//
//   gemm_tile_d      128 x 128 tile, 8 waves, LDS-DMA staging, K = 512 x (number of panels): the trailing updates of
//                    the blocked Cholesky (cho_factor, src/joint_prediction.py:69: k_syrk_group_d), of the forward
//                    substitution (first half of cho_solve, :68-73: k_aux_group_d) and of the Schur complement of
//                    the prediction sites (_verify_model, :260-274: k_schur_syrk_d) -- the dense contractions of the path.
//   gemm_tile_e      the same tile staged through registers for plain pointers and small K (k_gemm_nt_e: K = 64
//                    updates inside a panel; k_lt_update: the local predictor's trailing updates).
//   gemm_tile<2>     256 x 64 tile for the narrow panel-internal products (k_gemm_nt<2>).
//   k_potrf64        Cholesky of a 64 x 64 diagonal block AND its inverse (one workgroup, register resident).
//   k_trsm64m        row solves X L^T = A as a product with that inverse on the matrix cores.
//   k_panel_* / lt_* fused 64-column steps (right-hand-side rows of a panel; local predictor's tiled path).
//   k_reduce_pred    fused prediction / variance reductions (src/joint_prediction.py:74-78 without the m x m matrix).
//   k_tri_matvec     z = L eps (sim.py:52-54);  k_loo_rows: unit right-hand sides of the leave-one-out sweep.
//
// All matrices are row-major.  Dimensions handed to these kernels are padded by the host (ck_api.hip) so that no
// edge predication is needed in the hot loops.
#include "ck_internal.h"
#include "ck_tilemap.h"

typedef double d4_t __attribute__((ext_vector_type(4)));
typedef double d2_t __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------
// MFMA GEMM:  C (M x N) -= A (M x K) * B (N x K)^T
// ---------------------------------------------------------------------------------------
// Workgroup tile 256 x BN (BN = 128 or 64), K step 16, 512 threads = 8 waves laid out
// 4 (M) x 2 (N); each wave owns 64 x (BN/2) = 4 x WN MFMA tiles of 16 x 16, i.e. 16 or 8
// independent accumulators.  One wave per SIMD already saturates the f64 MFMA pipe when it
// issues back to back (measured by ck_debug_mfma_peak: 64 cycles per v_mfma_f64_16x16x4_f64,
// 77.8 TFLOP/s chip-wide), so everything else in the loop only has to stay out of the way.
//
// v_mfma_f64_16x16x4_f64 operand map (probed by ck_debug_mfma_probe): lane l supplies
// A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; result register r of lane l is
// D[row = (l >> 4) + 4 r][col = l & 15].  The contraction index of one MFMA may be ANY four
// k as long as A and B agree, so lane group g = l >> 4 reads the two CONSECUTIVE k = 2g, 2g + 1
// of an 8-wide k block with one ds_read_b128 and feeds them to two MFMAs.
//
// LDS image of a K step (16 k = 8 k-pairs p): plane p holds the 16-byte pair p of every row,
// rows XOR-swizzled by p in their low 3 bits:   byte(row, p) = p * rows * 16 + (row ^ p) * 16.
//   - staging writes (ds_write_b128, 8 consecutive lanes = the 8 pairs of ONE row, so the global
//     loads stay coalesced in full 128-byte lines) land on 8 distinct rows -> conflict free;
//   - operand reads (ds_read_b128, serviced in the fixed 16-lane groups of the hardware) cover
//     all 64 banks exactly once per group -> conflict free.
// C is loaded into the accumulators up front and A is negated on its way into LDS
// (acc = C + (-A) B^T), so the epilogue is stores only.
#define GEMM_BK 16

// A pointer LOADED from memory (sigptr[J]) is a generic pointer to hipcc: accesses through it become
// flat_load / flat_store, and a flat access counts on lgkmcnt as well as vmcnt -- every
// s_waitcnt lgkmcnt(0) in front of the MFMAs (meant for the ds_reads) would then also wait for the
// global prefetch of the next chunk.  as_global() puts such pointers back into the global address space.
typedef __attribute__((address_space(1))) char ck_gchar;
typedef __attribute__((address_space(1))) double ck_gdouble;
typedef __attribute__((address_space(1))) d2_t ck_gd2;
__device__ __forceinline__ const ck_gchar* as_global(const char* p) { return (const ck_gchar*)(unsigned long long)p; }
__device__ __forceinline__ ck_gchar* as_global(char* p) { return (ck_gchar*)(unsigned long long)p; }

template <int WN>
__device__ __forceinline__ void gemm_tile(double* __restrict__ C, long ldc, const double* __restrict__ A, long lda,
                                          const double* __restrict__ B, long ldb, long r0, long c0, int K,
                                          char* lds) {
    constexpr int BN = WN * 32;
    constexpr int BCH = BN * 8 / 512;            // 16-byte chunks of the B tile per thread (2 or 1)
    constexpr int PLANE_A = CK_BM * 16;          // bytes per k-pair plane
    constexpr int PLANE_B = BN * 16;
    constexpr int BOFF = 8 * PLANE_A;            // B planes follow the 8 A planes
    constexpr int STAGE = 8 * (PLANE_A + PLANE_B);

    const int tid = threadIdx.x;
    const int lane = tid & 63, w = tid >> 6;
    const int wm = w >> 1, wn = w & 1;
    const int li = lane & 15, g = lane >> 4;

    // Wave-uniform 64-bit bases + 32-bit per-thread offsets (saddr addressing: no 64-bit address
    // pairs in VGPRs; the accumulators need the room).
    const double* Ab = A + r0 * lda;
    const double* Bb = B + c0 * ldb;
    double* Cb = C + r0 * ldc + c0;
    // global -> register staging: chunk id -> (row = id >> 3, pair p = id & 7)
    unsigned a_src[4], b_src[BCH];
    int a_dst[4], b_dst[BCH];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int id = tid + 512 * u, row = id >> 3, p = id & 7;
        a_src[u] = (unsigned)(row * (int)lda + p * 2);
        a_dst[u] = p * PLANE_A + ((row ^ p) << 4);
    }
#pragma unroll
    for (int u = 0; u < BCH; ++u) {
        const int id = tid + 512 * u, row = id >> 3, p = id & 7;
        b_src[u] = (unsigned)(row * (int)ldb + p * 2);
        b_dst[u] = BOFF + p * PLANE_B + ((row ^ p) << 4);
    }
    const unsigned c_off = (unsigned)((wm * 64 + g) * (int)ldc + wn * (WN * 16) + li);

    // first K step in flight while C streams into the accumulators
    d2_t ra[4], rb[BCH];
#pragma unroll
    for (int u = 0; u < 4; ++u) ra[u] = *reinterpret_cast<const d2_t*>(Ab + a_src[u]);
#pragma unroll
    for (int u = 0; u < BCH; ++u) rb[u] = *reinterpret_cast<const d2_t*>(Bb + b_src[u]);

    d4_t acc[4][WN];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double* rowp = Cb + (long)(i * 16 + 4 * r) * ldc;   // wave-uniform -> SGPR base
#pragma unroll
            for (int j = 0; j < WN; ++j) acc[i][j][r] = rowp[c_off + j * 16];
        }

#pragma unroll
    for (int u = 0; u < 4; ++u) *reinterpret_cast<d2_t*>(lds + a_dst[u]) = -ra[u];
#pragma unroll
    for (int u = 0; u < BCH; ++u) *reinterpret_cast<d2_t*>(lds + b_dst[u]) = rb[u];
    // Drain the C loads HERE.  Otherwise the first MFMA of the loop body carries an
    // s_waitcnt vmcnt(0) for them on every iteration, which also waits for the next K step's
    // prefetch loads issued just above it and so serialises load latency with the MFMAs.
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();

    // operand read offsets for the two 8-wide k blocks (kb = 0, 1): pair p = 4 kb + g
    int a_rd[2], b_rd[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
        const int p = 4 * kb + g;
        a_rd[kb] = p * PLANE_A + ((wm * 64 + (li ^ p)) << 4);
        b_rd[kb] = BOFF + p * PLANE_B + ((wn * (WN * 16) + (li ^ p)) << 4);
    }

    const int nst = K / GEMM_BK;
    for (int st = 0; st < nst; ++st) {
        const int cur = st & 1;
        const bool more = (st + 1 < nst);
        if (more) {
            const int k0 = (st + 1) * GEMM_BK;
#pragma unroll
            for (int u = 0; u < 4; ++u) ra[u] = *reinterpret_cast<const d2_t*>(Ab + k0 + a_src[u]);
#pragma unroll
            for (int u = 0; u < BCH; ++u) rb[u] = *reinterpret_cast<const d2_t*>(Bb + k0 + b_src[u]);
        }
        const char* sb = lds + cur * STAGE;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            d2_t af[4], bf[WN];
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = *reinterpret_cast<const d2_t*>(sb + a_rd[kb] + i * 256);
#pragma unroll
            for (int j = 0; j < WN; ++j) bf[j] = *reinterpret_cast<const d2_t*>(sb + b_rd[kb] + j * 256);
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < WN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i][h], bf[j][h], acc[i][j], 0, 0, 0);
        }
        if (more) {
            char* nx = lds + (cur ^ 1) * STAGE;
#pragma unroll
            for (int u = 0; u < 4; ++u) *reinterpret_cast<d2_t*>(nx + a_dst[u]) = -ra[u];
#pragma unroll
            for (int u = 0; u < BCH; ++u) *reinterpret_cast<d2_t*>(nx + b_dst[u]) = rb[u];
        }
        __syncthreads();
    }

    // epilogue: stores only.  Register r of lane l is D[(l >> 4) + 4 r][l & 15].
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double* rowp = Cb + (long)(i * 16 + 4 * r) * ldc;
#pragma unroll
            for (int j = 0; j < WN; ++j) rowp[c_off + j * 16] = acc[i][j][r];
        }
}

// address-space-qualified void pointers for the LDS-DMA builtins
typedef __attribute__((address_space(3))) void ck_lds_void;

// (Two further schedules of the 256 x 128 tile were measured and removed: padded LDS rows with
// compiler-merged ds_read2_b64 operand reads -- 42 % of the LDS cycles were bank conflicts, 51.7 TF --
// and a ping-pong schedule, two wave groups alternating MFMA and memory phases over three LDS-DMA
// staged buffers, 48.5 TF.  DESIGN.md section 5 has the numbers.)

// XCD-aware bijective remap of a 1-D block id: blocks b and b + 8 share an XCD (and its L2);
// give each XCD a contiguous run of tiles so that neighbouring tiles (same A rows) meet in one L2.
__device__ __forceinline__ int xcd_remap(int b, int nblk) {
    const int xcd = b & 7, qq = nblk >> 3, rr = nblk & 7;
    return (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (b >> 3);
}

// ---------------------------------------------------------------------------------------
// 128 x 128 tile, 8 waves of 64 x 32, register-staged (plain pointers, any K % 16 == 0)
// ---------------------------------------------------------------------------------------
// The tile of the small-K products: the K = 64 panel-internal updates (k_gemm_nt_e) and the trailing updates
// of the local predictor's tiled path (k_lt_update).  A tile's C traffic (load 128 KB, store 128 KB) cannot
// overlap its own MFMA work -- the accumulators ARE the C tile -- so two independent workgroups share a CU
// (64 KB of LDS each) and drift out of phase: one's prologue / epilogue runs under the other's K loop.  Each
// wave owns a 64 x 32 quarter-strip (8 accumulator tiles = 64 VGPRs).  "Row image" LDS layout: 128-byte rows,
// 16-byte k-pair p of row r in slot p ^ ((r >> 1) & 7), filled through registers (coalesced 128-byte global
// rows, A negated on its way in), read with ds_read_b128 that hit every bank once per hardware lane group.
// CLIP: a wave whose 64 x 32 block lies entirely outside [0, row_lim) x [0, col_lim), or (lower) entirely above the
// diagonal, skips its C traffic and its MFMAs (it still stages its share of the operands): the ragged systems of the
// local predictor have a diagonal tile in every tile row and an overhang of up to 64 rows / columns.
template <bool CLIP>
__device__ __forceinline__ void gemm_tile_e(double* __restrict__ C, long ldc, const double* __restrict__ A, long lda,
                                            const double* __restrict__ B, long ldb, long r0, long c0, int K,
                                            char* lds, long row_lim = 0, long col_lim = 0, bool lower = false) {
    constexpr int BOFF = 128 * 128;              // B rows follow the 128 A rows
    constexpr int STAGE = 256 * 128;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = w >> 2, wn = w & 3;
    const int li = lane & 15, g = lane >> 4;
    const long wr = r0 + wm * 64, wc = c0 + wn * 32;
    const bool active = !CLIP || (wr < row_lim && wc < col_lim && !(lower && wc > wr + 63));   // wave-uniform (scalar)

    ck_gdouble* Cb = (ck_gdouble*)as_global(reinterpret_cast<char*>(C + r0 * ldc + c0));
    // Operand loads as buffer_load_dwordx4: the tile's A / B rows in a resource descriptor (scalar), one 32-bit offset
    // register per load (constant over the K loop), the chunk's byte offset as the scalar offset -- like the DMA tile, no
    // vector instruction in the MFMA loop that is not a load, a fragment read or an LDS write: the sign of A moved into the
    // accumulators (they start as -C and are stored as -acc), the LDS stage is a compile-time constant (two chunks per
    // iteration).  Rounds 1-3 had, per chunk and wave, four 64-bit address adds, six LDS address adds and eight
    // instructions for the negation in this loop; in gemm_tile_d the ten of them cost 4 % of the kernel.
    const __amdgpu_buffer_rsrc_t rsA =
        __builtin_amdgcn_make_buffer_rsrc((void*)(A + r0 * lda), (short)0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB =
        __builtin_amdgcn_make_buffer_rsrc((void*)(B + c0 * ldb), (short)0, 0x7fffffff, 0x00020000);
    // staging: chunk (row = tid >> 3 (+64 u), pair p = tid & 7) -> slot p ^ ((row >> 1) & 7); row + 64 u keeps the swizzle
    const int srow = tid >> 3, sp = tid & 7;
    unsigned a_off[2], b_off[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        a_off[u] = (unsigned)((srow + 64 * u) * (int)lda + sp * 2) * 8u;
        b_off[u] = (unsigned)((srow + 64 * u) * (int)ldb + sp * 2) * 8u;
    }
    const int s_dst0 = srow * 128 + ((sp ^ ((srow >> 1) & 7)) << 4);
    const unsigned c_off = (unsigned)((wm * 64 + g) * (int)ldc + wn * 32 + li) * 8u;
    int a_rd[2], b_rd[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
        const int slot = (4 * kb + g) ^ (li >> 1);
        a_rd[kb] = (wm * 64 + li) * 128 + slot * 16;
        b_rd[kb] = BOFF + (wn * 32 + li) * 128 + slot * 16;
    }
    typedef unsigned v4u_t __attribute__((ext_vector_type(4)));
    v4u_t ra[2], rb[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        ra[u] = __builtin_amdgcn_raw_buffer_load_b128(rsA, (int)a_off[u], 0, 0);
        rb[u] = __builtin_amdgcn_raw_buffer_load_b128(rsB, (int)b_off[u], 0, 0);
    }
    d4_t acc[4][2];
    if (active) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const ck_gchar* rowp = reinterpret_cast<const ck_gchar*>(Cb + (long)(i * 16 + 4 * r) * ldc);   // wave-uniform
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j][r] = -*reinterpret_cast<const ck_gdouble*>(rowp + j * 128 + c_off);
            }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        *reinterpret_cast<v4u_t*>(lds + s_dst0 + u * 8192) = ra[u];
        *reinterpret_cast<v4u_t*>(lds + BOFF + s_dst0 + u * 8192) = rb[u];
    }
    __builtin_amdgcn_s_waitcnt(0);   // C loads drained here, not inside the loop (see gemm_tile)
    __syncthreads();

    const int nst = K / GEMM_BK;
    auto step = [&](auto cur_c, int st) __attribute__((always_inline)) {
        constexpr int cur = decltype(cur_c)::value;
        const bool more = (st + 1 < nst);
        if (more) {
            const int kb_ = (st + 1) * (GEMM_BK * 8);   // byte offset of the next chunk inside a row
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                ra[u] = __builtin_amdgcn_raw_buffer_load_b128(rsA, (int)a_off[u], kb_, 0);
                rb[u] = __builtin_amdgcn_raw_buffer_load_b128(rsB, (int)b_off[u], kb_, 0);
            }
        }
        const char* sb = lds + cur * STAGE;
        if (active) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                d2_t af[4], bf[2];
#pragma unroll
                for (int i = 0; i < 4; ++i) af[i] = *reinterpret_cast<const d2_t*>(sb + a_rd[kb] + i * 2048);
#pragma unroll
                for (int j = 0; j < 2; ++j) bf[j] = *reinterpret_cast<const d2_t*>(sb + b_rd[kb] + j * 2048);
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i][h], bf[j][h], acc[i][j], 0, 0, 0);
            }
        }
        if (more) {
            char* nx = lds + (cur ^ 1) * STAGE;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                *reinterpret_cast<v4u_t*>(nx + s_dst0 + u * 8192) = ra[u];
                *reinterpret_cast<v4u_t*>(nx + BOFF + s_dst0 + u * 8192) = rb[u];
            }
        }
        __syncthreads();
    };
    int st = 0;
    for (; st + 1 < nst; st += 2) {
        step(std::integral_constant<int, 0>{}, st);
        step(std::integral_constant<int, 1>{}, st + 1);
    }
    if (st < nst) step(std::integral_constant<int, 0>{}, st);
    // The 16 row addresses are recomputed here from a laundered copy of the (wave-uniform) tile pointer: left to
    // itself hipcc keeps the prologue's sixteen 64-bit row pointers alive in VGPRs across the K loop for reuse
    // and, at the 128-VGPR budget of four waves per SIMD, spills them (22 VGPRs of scratch before this).
    ck_gdouble* Ce = Cb;
    asm volatile("" : "+s"(Ce));
    if (!active) return;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            ck_gchar* rowp = reinterpret_cast<ck_gchar*>(Ce + (long)(i * 16 + 4 * r) * ldc);
#pragma unroll
            for (int j = 0; j < 2; ++j) *reinterpret_cast<ck_gdouble*>(rowp + j * 128 + c_off) = -acc[i][j][r];
        }
}

__global__ __launch_bounds__(512, 4) void k_gemm_nt_e(double* __restrict__ C, long ldc, const double* __restrict__ A,
                                                       long lda, const double* __restrict__ B, long ldb, int tiles_m,
                                                       int tiles_n, int K, int lower, long diag_off, long sC, long sA,
                                                       long sB) {
    __shared__ __attribute__((aligned(16))) char lds[2 * 256 * 128];
    const int t = xcd_remap(blockIdx.x, tiles_m * tiles_n);
    const int tm = t / tiles_n, tn = t - tm * tiles_n;
    const long r0 = (long)tm * 128, c0 = (long)tn * 128;
    if (lower && r0 + 127 + diag_off < c0) return;
    const long y = blockIdx.y;
    gemm_tile_e<false>(C + y * sC, ldc, A + y * sA, lda, B + y * sB, ldb, r0, c0, K, lds);
}

// ---------------------------------------------------------------------------------------
// Multi-panel K: C -= sum_p A_p B_p^T in ONE pass over the C tile (option "panel_group")
// ---------------------------------------------------------------------------------------
// With K = 512 per trailing update, a 128 x 128 tile spends ~7 % of its time loading and storing C
// (accumulators = C tile; measured 61.7 TF at K = 512 against 65.5 at K = 2048 and 66.2 at K = 8192).  The
// factorisation therefore groups G panels (ck_api.hip: factor_sweep): the trailing matrix beyond a group is
// updated once with K = 512 G, its A / B operands coming from G different panel buffers: the source pointers
// change every 32 chunks (wave-uniform, scalar loads).  SRC::get(p, A, B): byte pointers to row r0 of A_p and
// row c0 of B_p (both ld = CK_NB doubles).

// operands of the grouped Cholesky trailing update: panels K0 .. K0 + np - 1, block column J.
// sigptr[K]: where panel K can be READ on this rank (its own storage, or the receive buffer a remote
// panel was broadcast into -- ck_api.hip: d_panelptr)
struct CkSrcSyrk {
    double* const* sigptr;
    int K0, J;
    long r0, c0;
    __device__ __forceinline__ void get(int p, const ck_gchar*& A, const ck_gchar*& B) const {
        const double* base = sigptr[K0 + p] + (long)(J - K0 - p) * CK_NB * CK_NB;
        A = as_global(reinterpret_cast<const char*>(base + r0 * CK_NB));
        B = as_global(reinterpret_cast<const char*>(base + c0 * CK_NB));
    }
};

// operands of the grouped right-hand-side update: aux block columns K0.., L panels K0.., target column J
struct CkSrcAux {
    const double* aux;
    long mpad;
    double* const* sigptr;
    int K0, J;
    long r0, c0;
    __device__ __forceinline__ void get(int p, const ck_gchar*& A, const ck_gchar*& B) const {
        A = as_global(reinterpret_cast<const char*>(aux + (long)(K0 + p) * mpad * CK_NB + r0 * CK_NB));
        B = as_global(reinterpret_cast<const char*>(sigptr[K0 + p] + (long)(J - K0 - p) * CK_NB * CK_NB + c0 * CK_NB));
    }
};

// ---------------------------------------------------------------------------------------
// The multi-panel tile: 128 x 128, 8 waves of 64 x 32, LDS-DMA staging -- the trailing updates of the
// factorisation, of the solve sweep and of the Schur complement
// ---------------------------------------------------------------------------------------
// The next chunk goes global -> LDS directly (LDS-DMA, 16 bytes per lane: one wave instruction fills 8 whole
// 128-byte rows, 1 KB linear in LDS; the row-image swizzle is applied on the GLOBAL side: lane (row r8, slot sj)
// fetches pair sj ^ ((row >> 1) & 7), so the global side stays one full line per row).  No staging registers, no
// ds_write, no sign flips in the loop: the accumulators start as -C and are stored as -acc.  Against the same
// tile staged through registers (global -> VGPR -> negate -> ds_write, waited for in front of each barrier):
// -10 ms in the factorisation and -8 ms in the solve sweep at N = 40 000.  Tile structures measured and retired
// (DESIGN.md section 5 keeps their numbers): 4 waves of 64 x 64 (register- and DMA-staged), 128 x 64 tiles with
// three workgroups per CU, one 256 x 128 workgroup per CU, padded LDS rows, a ping-pong schedule.
// NI: 16-row blocks this WAVE computes (4: all of its 64 rows).  A right-hand-side tile row that holds only a few rows in front of
// the padding (m + 1 = 8 834 rows: 69 tile rows and two rows) runs with NI = 1 in the waves of the upper half and NI = 0 -- staging
// and barriers only -- in the others (k_tall_group_d): an eighth of a tile's MFMAs; a row's result does not depend on its neighbours.
// RANK1 (k_ginv_syrk_d): the accumulators start from ar[row] ac[col] instead of the C tile (which is then written, not read);
// rq > 1 (ck_loglik_reml): from sum_j ar[j rld + row] ac[j rld + col] over rq vector pairs, the first product as for rq = 1
// SCATTER (k_draw_trmm): the tile's column c is stored to column cmap[c] of C (none where cmap[c] < 0), its rows only in front
// of row_lim; C is then the output's base (c0 plays no part in the store)
// GRAM (k_fold_gram): the 128 A rows and the 128 B rows are GATHERED -- image row r of the tile is row src.ga[r] / src.gb[r] of the
// source panel, so SRC::get returns the panel's row 0 and a transfer's per-lane offset register carries the row (one panel row is
// CK_NB contiguous doubles: every transfer still fetches whole 128-byte lines); the accumulators start from zero and C = + A B^T
// is written, not read
template <int WAVES, class SRC, int NI = 4, bool RANK1 = false, bool SCATTER = false, bool GRAM = false>
__device__ __forceinline__ void gemm_tile_d(double* __restrict__ C, long ldc, const SRC& src, int np, long r0, long c0,
                                            char* lds, const double* __restrict__ ar = nullptr,
                                            const double* __restrict__ ac = nullptr, const int* __restrict__ cmap = nullptr,
                                            long row_lim = 0, int rq = 1, long rld = 0) {
    static_assert(WAVES == 8, "8 waves of 64 x 32");
    constexpr int NA = NI > 0 ? NI : 1;
    constexpr int BOFF = 128 * 128;
    constexpr int STAGE = 256 * 128;
    constexpr int NST = CK_NB / GEMM_BK;
    constexpr int WCOLS = WAVES == 8 ? 4 : 2;    // waves across the tile's columns
    constexpr int WJ = 128 / WCOLS / 16;         // 16-column MFMA tiles per wave
    constexpr int RPW = 256 / WAVES;             // image rows each wave stages per chunk
    constexpr int NDMA = RPW / 8;                // DMA instructions per wave and chunk
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = w / WCOLS, wn = w % WCOLS;
    const int li = lane & 15, g = lane >> 4;

    ck_gdouble* Cb = (ck_gdouble*)as_global(reinterpret_cast<char*>(C + r0 * ldc + c0));
    const unsigned c_off = (unsigned)((wm * 64 + g) * (int)ldc + wn * (WJ * 16) + li) * 8u;
    int a_rd[2], b_rd[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
        const int slot = (4 * kb + g) ^ (li >> 1);
        a_rd[kb] = (wm * 64 + li) * 128 + slot * 16;
        b_rd[kb] = BOFF + (wn * (WJ * 16) + li) * 128 + slot * 16;
    }
    // DMA duty of wave w: image rows [RPW w, RPW w + RPW) -- A rows for the first half of the waves, B rows
    // for the second -- as NDMA instructions of 8 rows; lane -> (row r8 = lane >> 3, slot sj = lane & 7)
    const int r8 = lane >> 3, sj = lane & 7;
    const bool stage_a = w < WAVES / 2;
    const unsigned d_row = (unsigned)((RPW * (w % (WAVES / 2)) + r8) * CK_NB) * 8u;
    const unsigned d_even = d_row + 16u * (unsigned)(sj ^ (r8 >> 1));
    const unsigned d_odd = d_row + 16u * (unsigned)(sj ^ (r8 >> 1) ^ 4);
    char* const lds_w = lds + RPW * w * 128;

    const ck_gchar *Ab, *Bb;
    src.get(0, Ab, Bb);
    // The transfers are buffer_load_dwordx4 ... lds: the panel rows' base in a resource descriptor (scalar registers, rebuilt
    // when the source panel changes), one 32-bit offset register per transfer (constant over the K loop) and the chunk's
    // byte offset as the scalar offset -- no vector instruction per transfer and one address register instead of the two of
    // global_load_lds_dwordx4 with its 64-bit per-lane address (rounds 1-3: a v_lshl_add_u64 in front of every transfer):
    // trailing updates 299.6 -> 297.3 ms per factorisation at N = 40 000, two interleaved pairs of runs.
    unsigned vo4[NDMA];
#pragma unroll
    // (the four transfers of a chunk share one LDS base in M0: the instruction's immediate offset, 0 / 1024 / 2048 / 3072, counts
    // on the LDS side AND on the memory side, so the per-lane offset registers carry the difference)
    for (int t = 0; t < NDMA; ++t) {
        if constexpr (GRAM) {   // (a gathered row is at least row 1 of the panel: the offset stays positive behind the - t * 1024)
            const int ir = RPW * (w % (WAVES / 2)) + 8 * t + r8;
            const unsigned grow = (unsigned)(stage_a ? src.ga[ir] : src.gb[ir]);
            vo4[t] = grow * (unsigned)(CK_NB * 8) + 16u * (unsigned)(sj ^ (r8 >> 1) ^ ((t & 1) ? 4 : 0)) - (unsigned)(t * 1024);
        } else {
            vo4[t] = ((t & 1) ? d_odd : d_even) + (unsigned)(8 * t * CK_NB) * 8u - (unsigned)(t * 1024);
        }
    }
#define CK_DMA_CHUNK(stage_, kbyte_)                                                                            \
    {                                                                                                           \
        const __amdgpu_buffer_rsrc_t rs_ = __builtin_amdgcn_make_buffer_rsrc(                                   \
            (void*)(unsigned long long)(stage_a ? Ab : Bb), (short)0, 0x7fffffff, 0x00020000);                  \
        ck_lds_void* lp_ = (ck_lds_void*)(lds_w + (stage_) * STAGE);                                            \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_, lp_, 16, (int)vo4[0], (int)(kbyte_), 0, 0);               \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_, lp_, 16, (int)vo4[1], (int)(kbyte_), 1024, 0);            \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_, lp_, 16, (int)vo4[2], (int)(kbyte_), 2048, 0);            \
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_, lp_, 16, (int)vo4[3], (int)(kbyte_), 3072, 0);            \
    }
    CK_DMA_CHUNK(0, 0L);
    d4_t acc[NA][WJ];
    if constexpr (GRAM) {
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < WJ; ++j) acc[i][j] = d4_t{0.0, 0.0, 0.0, 0.0};
    } else if constexpr (RANK1) {
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double a = ar[wm * 64 + g + i * 16 + 4 * r];
#pragma unroll
                for (int j = 0; j < WJ; ++j) {
                    if (rq == 1) {   // (a compile-time 1 everywhere but k_ginv_syrk_d<true>: the rank-1 code as it was)
                        acc[i][j][r] = -(a * ac[wn * (WJ * 16) + j * 16 + li]);
                        continue;
                    }
                    double s = a * ac[wn * (WJ * 16) + j * 16 + li];
                    for (int v = 1; v < rq; ++v)
                        s += ar[v * rld + wm * 64 + g + i * 16 + 4 * r] * ac[v * rld + wn * (WJ * 16) + j * 16 + li];
                    acc[i][j][r] = -s;
                }
            }
    } else {
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const ck_gchar* rowp = reinterpret_cast<const ck_gchar*>(Cb + (long)(i * 16 + 4 * r) * ldc);   // wave-uniform
#pragma unroll
                for (int j = 0; j < WJ; ++j) acc[i][j][r] = -*reinterpret_cast<const ck_gdouble*>(rowp + j * 128 + c_off);
            }
    }
    __builtin_amdgcn_s_waitcnt(0);   // C and the first chunk have landed
    __syncthreads();

    // (Tried: s_setprio 1 around the chunk's MFMAs -- 1 % slower.)
    // The DMA of chunk st + 2 is issued right BEHIND the barrier of chunk st -- into the stage chunk st has just been read
    // from -- and waited for in front of the barrier of chunk st + 1.  hipcc sinks the second half of a chunk's MFMAs below
    // its barrier, so with the DMA issued at the TOP of the next iteration (rounds 1-2) a transfer had only the first
    // half-chunk's 16 MFMAs to land; issued here it has a whole chunk (32 MFMAs) and still needs no third LDS stage.
    const int nst = np * NST;
    int pnl = 0, kc = 0;             // panel and chunk-in-panel of the chunk being PREFETCHED
#define CK_DMA_NEXT(stage_)                                   \
    {                                                         \
        if (++kc == NST) {                                    \
            kc = 0;                                           \
            src.get(++pnl, Ab, Bb);                           \
        }                                                     \
        CK_DMA_CHUNK((stage_), (long)kc * (GEMM_BK * 8));     \
    }
    if (nst > 1) CK_DMA_NEXT(1);     // chunk 1 (chunk 0 has landed: waited for above)
    // The loop runs two chunks per iteration (the number of chunks is a multiple of 32), so that the LDS stage of a chunk
    // is a compile-time constant: the fragment reads take it as the immediate offset of ds_read_b128 instead of six vector
    // instructions per chunk that add it to the per-lane addresses.
    // Two fragment sets: the reads of a half-chunk's fragments are issued in front of the OTHER half-chunk's sixteen MFMAs --
    // the second half's (same stage) in front of the first half's MFMAs, the next chunk's first half (other stage, visible
    // since this chunk's barrier) in front of the second half's -- so that no LDS round trip is exposed.  (Tried in round 3's
    // first session with the barrier in mid-chunk: 3 % slower then, with ten vector instructions still in the loop; now
    // trailing updates 287.8 -> 285.8 ms per factorisation.)
    d2_t af0[NA], bf0[WJ], af1[NA], bf1[WJ];
#pragma unroll
    for (int i = 0; i < NI; ++i) af0[i] = *reinterpret_cast<const d2_t*>(lds + a_rd[0] + i * 2048);
    if (NI > 0)
#pragma unroll
        for (int j = 0; j < WJ; ++j) bf0[j] = *reinterpret_cast<const d2_t*>(lds + b_rd[0] + j * 2048);
    auto step = [&](auto cur_c, int st) __attribute__((always_inline)) {
        constexpr int cur = decltype(cur_c)::value;
        const char* sb = lds + cur * STAGE;
        const char* sn = lds + (cur ^ 1) * STAGE;
#pragma unroll
        for (int i = 0; i < NI; ++i) af1[i] = *reinterpret_cast<const d2_t*>(sb + a_rd[1] + i * 2048);
        if (NI > 0)
#pragma unroll
            for (int j = 0; j < WJ; ++j) bf1[j] = *reinterpret_cast<const d2_t*>(sb + b_rd[1] + j * 2048);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < WJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af0[i][h], bf0[j][h], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_s_waitcnt(0x0070);   // vmcnt(0) lgkmcnt(0): the next chunk has landed, this stage has been read
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        if (st + 2 < nst) CK_DMA_NEXT(cur);
        if (st + 1 < nst) {
#pragma unroll
            for (int i = 0; i < NI; ++i) af0[i] = *reinterpret_cast<const d2_t*>(sn + a_rd[0] + i * 2048);
            if (NI > 0)
#pragma unroll
                for (int j = 0; j < WJ; ++j) bf0[j] = *reinterpret_cast<const d2_t*>(sn + b_rd[0] + j * 2048);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < WJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af1[i][h], bf1[j][h], acc[i][j], 0, 0, 0);
    };
    for (int st = 0; st < nst; st += 2) {
        step(std::integral_constant<int, 0>{}, st);
        step(std::integral_constant<int, 1>{}, st + 1);
    }
#undef CK_DMA_NEXT
#undef CK_DMA_CHUNK
    if constexpr (SCATTER) {
        int col[WJ];
#pragma unroll
        for (int j = 0; j < WJ; ++j) col[j] = cmap[wn * (WJ * 16) + j * 16 + li];
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row = r0 + wm * 64 + g + i * 16 + 4 * r;
                if (row >= row_lim) continue;
#pragma unroll
                for (int j = 0; j < WJ; ++j)
                    if (col[j] >= 0) C[row * ldc + col[j]] = -acc[i][j][r];
            }
        return;
    }
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            ck_gchar* rowp = reinterpret_cast<ck_gchar*>(Cb + (long)(i * 16 + 4 * r) * ldc);
#pragma unroll
            for (int j = 0; j < WJ; ++j) *reinterpret_cast<ck_gdouble*>(rowp + j * 128 + c_off) = GRAM ? acc[i][j][r] : -acc[i][j][r];
        }
}

// STAMP (diagnostic, ck_debug_gemm_clock / ck_debug_gemm_stamps): thread 0 of every workgroup leaves the shader cycles and
// the 100 MHz ticks of its lifetime in stamps[4 b], stamps[4 b + 1], then its start in 100 MHz ticks and XCC_ID << 32 |
// HW_ID.  cycles / ticks is the clock the chip holds under this kernel on this data (MI355X lowers its clock under load
// by an amount that depends on the operands: MI355X_MICROARCH.md, "DVFS give-back"); starts and lifetimes show how many
// of the chip's 512 tile slots are occupied over a launch.
template <int WAVES, bool STAMP = false>
__global__ __launch_bounds__(WAVES * 64, WAVES == 8 ? 4 : 2) void k_syrk_group_d(double* const* __restrict__ sigptr,
                                                         double* const* __restrict__ srcptr, int K0, int np,
                                                         const CkTileMap map,
                                                         unsigned long long* __restrict__ stamps = nullptr) {
    __shared__ __attribute__((aligned(16))) char lds[2 * 256 * 128];
    unsigned long long t0 = 0, q0 = 0;
    if (STAMP) {
        t0 = __builtin_amdgcn_s_memtime();
        q0 = __builtin_amdgcn_s_memrealtime();
    }
    // one workgroup per tile, none that returns at once (ck_tilemap.h); every XCD a contiguous run of the launch's tiles
    int u, tm, tn;
    ck_tilemap_get(map, xcd_remap(blockIdx.x, (int)map.total), u, tm, tn);
    const int J = map.J0 + u * map.Jstep;
    const long r0 = (long)tm * 128, c0 = (long)tn * 128;
    const CkSrcSyrk src{srcptr, K0, J, r0, c0};
    gemm_tile_d<WAVES>(sigptr[J], CK_NB, src, np, r0, c0, lds);
    if (STAMP) {
        __builtin_amdgcn_s_waitcnt(0);
        const unsigned long long t1 = __builtin_amdgcn_s_memtime(), q1 = __builtin_amdgcn_s_memrealtime();
        if (threadIdx.x == 0) {
            const size_t b = blockIdx.x;
            stamps[4 * b] = t1 - t0;
            stamps[4 * b + 1] = q1 - q0;
            stamps[4 * b + 2] = q0;
            stamps[4 * b + 3] = ((unsigned long long)__builtin_amdgcn_s_getreg((3 << 11) | 20) << 32) |
                                __builtin_amdgcn_s_getreg((31 << 11) | 4);   // XCC_ID, HW_ID
        }
    }
}

template <int WAVES>
__global__ __launch_bounds__(WAVES * 64, WAVES == 8 ? 4 : 2) void k_aux_group_d(double* __restrict__ aux, long mpad,
                                                        double* const* __restrict__ sigptr, int K0, int np, int J0,
                                                        long mrows, long nvalid, int thin_tm) {
    __shared__ __attribute__((aligned(16))) char lds[2 * 256 * 128];
    const int J = J0 + (int)blockIdx.y;
    const int tiles_n = CK_NB / 128;
    const int nblk = (int)(mrows / 128) * tiles_n;   // the first mrows of the mpad rows (the others are known zeros)
    const int t = xcd_remap(blockIdx.x, nblk);
    const int tm = t / tiles_n, tn = t - tm * tiles_n;
    const long r0 = (long)tm * 128, c0 = (long)tn * 128;
    if ((long)J * CK_NB + c0 >= nvalid) return;   // columns of the identity padding: the rows of L there are zero
    const CkSrcAux src{aux, mpad, sigptr, K0, J, r0, c0};
    double* C = aux + (long)J * mpad * CK_NB;
    if (tm != thin_tm) {   // (thin_tm: see k_tall_group_d)
        gemm_tile_d<WAVES>(C, CK_NB, src, np, r0, c0, lds);
    } else if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) < 4) {
        gemm_tile_d<WAVES, CkSrcAux, 1>(C, CK_NB, src, np, r0, c0, lds);
    } else {
        gemm_tile_d<WAVES, CkSrcAux, 0>(C, CK_NB, src, np, r0, c0, lds);
    }
}

// ---------------------------------------------------------------------------------------
// The TALL matrix [Sigma; c0^T; z^T] (round 4): one launch per update, triangle and right-hand-side tiles together
// ---------------------------------------------------------------------------------------
// The forward substitution of the right-hand-side rows IS the panel step applied to more rows, and a
// block column's right-hand-side tiles take the same B operand rows (L panel rows of block column J) as its triangle tiles.
// Rounds 1-3 ran them as two kernels (k_syrk_group_d, k_aux_group_d) -- in ck_factor_predict on two streams that share the
// chip, 156 launches per pass, each with its own fill and drain, the one-column right-hand-side launches filling 280 of 512
// slots.  Here a launch's grid is the tiles of both (ck_tilemap.h: axr), column by column, so that a block column's B rows
// meet all their readers in one XCD's L2.  Every tile computes exactly what it computed before (same operands, same K
// order): the results keep their bits.
struct CkSrcTall {
    double* const* sigptr;
    const double* aux;
    long mpad;
    int K0, J;
    long r0, c0;
    bool ax;   // wave-uniform: this tile belongs to the right-hand-side block
    __device__ __forceinline__ void get(int p, const ck_gchar*& A, const ck_gchar*& B) const {
        const double* base = sigptr[K0 + p] + (long)(J - K0 - p) * CK_NB * CK_NB;
        const double* arow = ax ? aux + (long)(K0 + p) * mpad * CK_NB : base;
        A = as_global(reinterpret_cast<const char*>(arow + r0 * CK_NB));
        B = as_global(reinterpret_cast<const char*>(base + c0 * CK_NB));
    }
};

// thin_tm: the right-hand-side tile row with at most 16 rows in front of the padding (-1: none) -- gemm_tile_d's NI.  Its tiles are
// NOT part of the map (which then holds one right-hand-side tile row fewer): they are the last workgroups of the grid, dealt to the
// XCDs round-robin.  In launch order they finished in a third of a tile's time and put every later tile of their slot out of step
// with the tiles it shares operand rows with: FETCH_SIZE per launch rose by 45 % (21.6 -> 31.4 GB for the largest launch).
__global__ __launch_bounds__(512, 4) void k_tall_group_d(double* const* __restrict__ sigptr, double* __restrict__ aux, long mpad,
                                                          int K0, int np, const CkTileMap map, int thin_tm) {
    __shared__ __attribute__((aligned(16))) char lds[2 * 256 * 128];
    int u, tm, tn;
    bool ax;
    const bool thin = (long long)blockIdx.x >= map.total;   // block-uniform
    if (!thin) {
        ax = ck_tilemap_get(map, xcd_remap(blockIdx.x, (int)map.total), u, tm, tn);
    } else {
        const int q = (int)((long long)blockIdx.x - map.total);   // tile columns 0 .. 3 of the full block columns, then the short one's
        u = q >> 2 < map.nfull ? q >> 2 : map.nfull;
        tn = q - 4 * u;
        tm = thin_tm;
        ax = true;
    }
    const int J = map.J0 + u * map.Jstep;
    const long r0 = (long)tm * 128, c0 = (long)tn * 128;
    const CkSrcTall src{sigptr, aux, mpad, K0, J, r0, c0, ax};
    double* C = ax ? aux + (long)J * mpad * CK_NB : sigptr[J];
    if (!thin) {
        gemm_tile_d<8>(C, CK_NB, src, np, r0, c0, lds);
    } else if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) < 4) {   // the waves of rows 0 .. 63: their first 16-row block
        gemm_tile_d<8, CkSrcTall, 1>(C, CK_NB, src, np, r0, c0, lds);
    } else {                                                             // rows 64 .. 127 are padding: staging and barriers only
        gemm_tile_d<8, CkSrcTall, 0>(C, CK_NB, src, np, r0, c0, lds);
    }
}

// block columns J0 .. J0 + nJ - 1 of Sigma (lower tiles in front of the padding) and of the mpad right-hand-side rows, by the
// panels K0 .. K0 + np - 1 (single process: every panel in its own storage)
// mrows: right-hand-side rows in front of the padding (m + 1; <= 0: treat all mpad rows as live)
void ck_launch_tall_group(hipStream_t s, double* const* sigptr_dev, double* aux, int64_t mpad, int K0, int np, int J0, int nJ,
                          int64_t nvalid, int64_t mrows) {
    if (nJ <= 0 || np <= 0) return;
    const int axr = (int)(mpad / 128);
    const int thin_tm = mrows > 0 && mrows % 128 >= 1 && mrows % 128 <= 16 && mrows / 128 == axr - 1 ? axr - 1 : -1;
    const CkTileMap map = ck_tilemap_make(nvalid, J0, 1, nJ, thin_tm >= 0 ? axr - 1 : axr);
    if (map.total <= 0) return;
    const long long nthin = thin_tm >= 0 ? 4LL * map.nfull + map.tv_last : 0;
    k_tall_group_d<<<dim3((unsigned)(map.total + nthin)), dim3(512), 0, s>>>(sigptr_dev, aux, (long)mpad, K0, np, map, thin_tm);
}

// Schur complement of the prediction sites, S = C_pp - V^T V (ck_verify_model): the solved right-hand-side rows
// V^T (one row per prediction site, block column p of the data sites at aux + p * mpad * NB) are both operands;
// block column J of S (rows J * NB .., packed like a Sigma panel) -= sum over ALL np data block columns in one
// launch (K = np * 512: the C tile is read and written once).
struct CkSrcSchur {
    const double* aux;
    long mpad;
    int J;
    long r0, c0;
    __device__ __forceinline__ void get(int p, const ck_gchar*& A, const ck_gchar*& B) const {
        const double* base = aux + (long)p * mpad * CK_NB + (long)J * CK_NB * CK_NB;
        A = as_global(reinterpret_cast<const char*>(base + r0 * CK_NB));
        B = as_global(reinterpret_cast<const char*>(base + c0 * CK_NB));
    }
};

__global__ __launch_bounds__(512, 4) void k_schur_syrk_d(double* const* __restrict__ schur, const double* __restrict__ aux,
                                                          long mpad, int np, const CkTileMap map) {
    __shared__ __attribute__((aligned(16))) char lds[2 * 256 * 128];
    int u, tm, tn;   // one workgroup per tile on or below the diagonal, in front of the rows beyond the right-hand-side storage
    ck_tilemap_get(map, xcd_remap(blockIdx.x, (int)map.total), u, tm, tn);
    const int J = map.J0 + u * map.Jstep;
    const long r0 = (long)tm * 128, c0 = (long)tn * 128;
    const CkSrcSchur src{aux, mpad, J, r0, c0};
    gemm_tile_d<8>(schur[J], CK_NB, src, np, r0, c0, lds);
}

void ck_launch_schur_syrk(hipStream_t s, double* const* schur_dev, const double* aux, int64_t mpad, int np, int nJ,
                          int64_t Mpad) {
    if (nJ <= 0 || np <= 0) return;
    // rows from floor(mpad / 128) * 128 on are beyond the right-hand-side storage: padding, stays identity
    const CkTileMap map = ck_tilemap_make(std::min<int64_t>(mpad / 128 * 128, Mpad), 0, 1, nJ);
    if (map.total <= 0) return;
    k_schur_syrk_d<<<dim3((unsigned)map.total), dim3(512), 0, s>>>(schur_dev, aux, mpad, np, map);
}

// G = alpha alpha^T - Sigma^-1 of the log-likelihood's gradient (ck_loglik), lower triangle in packed block columns like the
// Schur complement above.  W: the solved unit right-hand-side rows of ALL data sites, row 1 + p = (L^-1 e_p)^T (row 0 = y),
// so (Sigma^-1)_pq = W_p . W_q; alpha_p = W_p . y.  W_p is zero in every column before p (L^-1 is lower triangular): a tile
// whose first row is p0 needs the panels from p0 / NB on only (the rows are the larger index of a lower tile), so the launch
// performs N^3 / 3 flop instead of N^3.  The accumulators start from the rank-1 term (gemm_tile_d, RANK1).
struct CkSrcGinv {
    const double* aux;
    long mpad;
    int K0;
    long ra, rb;   // aux rows of the tile's first row / column (1 + index)
    __device__ __forceinline__ void get(int p, const ck_gchar*& A, const ck_gchar*& B) const {
        const double* base = aux + (long)(K0 + p) * mpad * CK_NB;
        A = as_global(reinterpret_cast<const char*>(base + ra * CK_NB));
        B = as_global(reinterpret_cast<const char*>(base + rb * CK_NB));
    }
};

// RQ = false (ck_loglik, and ck_loglik_reml without a trend): the rank-1 start with rq a compile-time 1 -- the code of the ML path
// is the rank-1 kernel's; RQ = true: the rank-q start of ck_loglik_reml (q = 1 + p at run time)
template <bool RQ>
__global__ __launch_bounds__(512, 4) void k_ginv_syrk_d(double* const* __restrict__ G, const double* __restrict__ aux, long mpad,
                                                         const double* __restrict__ alpha, int nK, const CkTileMap map, int q,
                                                         long ald, int dense) {
    __shared__ __attribute__((aligned(16))) char lds[2 * 256 * 128];
    int u, tm, tn;
    ck_tilemap_get(map, xcd_remap(blockIdx.x, (int)map.total), u, tm, tn);
    const int J = map.J0 + u * map.Jstep;
    const long r0 = (long)tm * 128, c0 = (long)tn * 128;
    const long p0 = (long)J * CK_NB + r0, q0 = (long)J * CK_NB + c0;
    const int K0 = (int)(p0 / CK_NB);
    const long dn = RQ ? dense : 1;   // (ck_loglik: one dense row, the data row)
    const CkSrcGinv src{aux, mpad, K0, dn + p0, dn + q0};
    gemm_tile_d<8, CkSrcGinv, 4, true>(G[J], CK_NB, src, nK - K0, r0, c0, lds, alpha + p0, alpha + q0, nullptr, 0, RQ ? q : 1,
                                       ald);
}

void ck_launch_ginv_syrk(hipStream_t s, double* const* G_dev, const double* aux, int64_t mpad, const double* avec, int nK,
                         int64_t nvalid, int q, int64_t ald, int dense) {
    if (nK <= 0) return;
    const CkTileMap map = ck_tilemap_make(nvalid, 0, 1, nK);
    if (map.total <= 0) return;
    if (q == 1)
        k_ginv_syrk_d<false><<<dim3((unsigned)map.total), dim3(512), 0, s>>>(G_dev, aux, mpad, avec, nK, map, 1, (long)ald, dense);
    else
        k_ginv_syrk_d<true><<<dim3((unsigned)map.total), dim3(512), 0, s>>>(G_dev, aux, mpad, avec, nK, map, q, (long)ald, dense);
}

// The products B = Sigma^-1 D of the Fisher information (ck_loglik_fisher, ck_fisher.hip): Sigma^-1 as full K-panels (Sp: panel
// P = npad rows of its 512 columns) against one unit of a derivative operand (ck_internal.h: CkFisherUnit), restricted to the
// panels and columns the unit lives in.  C starts at zero and receives -Sigma^-1 D (the tile's sign).
struct CkSrcFisher {
    const double* Sp;
    long npad;
    const double* D;
    long wpad;
    int pK0;
    long r0, c0;
    __device__ __forceinline__ void get(int p, const ck_gchar*& A, const ck_gchar*& B) const {
        A = as_global(reinterpret_cast<const char*>(Sp + ((long)(pK0 + p) * npad + r0) * CK_NB));
        B = as_global(reinterpret_cast<const char*>(D + ((long)p * wpad + c0) * CK_NB));
    }
};

__global__ __launch_bounds__(512, 4) void k_fisher_prod(double* __restrict__ C, long ldc, const double* __restrict__ Sp, long npad,
                                                         const double* __restrict__ D, long wpad, int pK0, int npan, int tiles_n) {
    __shared__ __attribute__((aligned(16))) char lds[2 * 256 * 128];
    const int t = xcd_remap(blockIdx.x, (int)gridDim.x);
    const int tm = t / tiles_n, tn = t - tm * tiles_n;
    const long r0 = (long)tm * 128, c0 = (long)tn * 128;
    const CkSrcFisher src{Sp, npad, D, wpad, pK0, r0, c0};
    gemm_tile_d<8>(C, ldc, src, npan, r0, c0, lds);
}

void ck_launch_fisher_prod(hipStream_t s, double* C, int64_t ldc, const double* Sp, int64_t npad, const double* D, int64_t wpad,
                           int pK0, int npan) {
    if (npad <= 0 || wpad <= 0 || npan <= 0) return;
    const int tiles_m = (int)(npad / 128), tiles_n = (int)(wpad / 128);
    k_fisher_prod<<<dim3((unsigned)(tiles_m * tiles_n)), dim3(512), 0, s>>>(C, (long)ldc, Sp, (long)npad, D, (long)wpad, pK0, npan,
                                                                          tiles_n);
}

// ---------------------------------------------------------------------------------------
// Leave-group-out cross-validation (ck_cv_folds): the Gram matrices Q_SS = W_S W_S^T of all folds in ONE launch
// ---------------------------------------------------------------------------------------
// W: the solved unit right-hand-side rows of the leave-one-out layout.  A fold's rows are scattered over the buffer, but a row's
// slice of a panel is CK_NB contiguous doubles, so the tile's operand loader takes the row from an index list (gemm_tile_d,
// GRAM) and everything behind the loader is the trailing updates' tile.  One workgroup per tile of the host's tile map
// (ck_host.cpp: ck_host_fold_plan): only within-fold tiles exist, and a tile starts at the panel of its first position -- in
// front of it its later operand is structurally zero.
struct CkSrcGram {
    const double* aux;
    long mpad;
    int K0;
    const int* ga;
    const int* gb;
    __device__ __forceinline__ void get(int p, const ck_gchar*& A, const ck_gchar*& B) const {
        A = as_global(reinterpret_cast<const char*>(aux + (long)(K0 + p) * mpad * CK_NB));
        B = A;
    }
};

__global__ __launch_bounds__(512, 4) void k_fold_gram(const double* __restrict__ aux, long mpad, int nK,
                                                       const CkFoldTile* __restrict__ tiles, const int* __restrict__ grow,
                                                       double* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) char lds[2 * 256 * 128];
    const CkFoldTile t = tiles[blockIdx.x];
    const int K0 = t.pos0 / CK_NB;
    const CkSrcGram src{aux, mpad, K0, grow + t.a0, grow + t.b0};
    gemm_tile_d<8, CkSrcGram, 4, false, false, true>(out + t.c_off, (long)t.ld, src, nK - K0, 0, 0, lds);
}

void ck_launch_fold_gram(hipStream_t s, const double* aux, int64_t mpad, int nK, const CkFoldTile* tiles, int64_t n_tiles,
                         const int* grow, double* out) {
    if (n_tiles <= 0) return;
    k_fold_gram<<<dim3((unsigned)n_tiles), dim3(512), 0, s>>>(aux, (long)mpad, nK, tiles, grow, out);
}

// Conditional simulation (ck_conditional_draws): X = pred + eps L_S^T for a chunk of draws, L_S the factor of the
// deflated posterior covariance in the Schur buffers (packed block columns, upper triangles of the diagonal blocks zeroed:
// ck_draws.hip k_draw_upper).  Output tile (draw rows r0.., sites k0..): X = sum over the block columns p <= k0 / NB of
// E_p L_S[k0.., p]^T -- the lower tiles only, K = NB (k0 / NB + 1), m^2 n_draws flop in all.  E holds -eps (ck_draws.hip:
// k_draw_noise) in the same block-column layout (ld NB, ldp rows per block column); the accumulators start from -pred
// (RANK1 with ar = ones) and are stored negated, so the tile is pred + eps L_S^T.  Every output element sums its K in the
// same order whatever the chunk of draws it lands in: the draws' bits do not depend on the chunking.
struct CkSrcDraw {
    const double* E;
    long ldp;
    double* const* L;
    long r0, k0;
    __device__ __forceinline__ void get(int p, const ck_gchar*& A, const ck_gchar*& B) const {
        A = as_global(reinterpret_cast<const char*>(E + (long)p * ldp * CK_NB + r0 * CK_NB));
        B = as_global(reinterpret_cast<const char*>(L[p] + (k0 - (long)p * CK_NB) * CK_NB));
    }
};

// one workgroup per 128 x 128 tile, the site tiles with the longest K first (blockIdx.x = tc_rev * tiles_r + tr)
__global__ __launch_bounds__(512, 4) void k_draw_trmm(double* __restrict__ X, long ldx, const double* __restrict__ E, long ldp,
                                                       double* const* __restrict__ L, const double* __restrict__ pred,
                                                       const double* __restrict__ ones, const int* __restrict__ cmap,
                                                       int tiles_r, int tiles_c, long nd) {
    __shared__ __attribute__((aligned(16))) char lds[2 * 256 * 128];
    const int tc = tiles_c - 1 - (int)(blockIdx.x / (unsigned)tiles_r);
    const int tr = (int)(blockIdx.x % (unsigned)tiles_r);
    const long r0 = (long)tr * 128, k0 = (long)tc * 128;
    const CkSrcDraw src{E, ldp, L, r0, k0};
    gemm_tile_d<8, CkSrcDraw, 4, true, true>(X, ldx, src, (int)(k0 / CK_NB) + 1, r0, 0, lds, ones, pred + k0, cmap + k0, nd);
}

// X: nd x m (the caller's site order, ld m); E: ldp x Mp in block columns; pred / cmap: Mp entries (cmap -1 beyond m)
void ck_launch_draw_trmm(hipStream_t s, double* X, int64_t m, const double* E, int64_t ldp, int64_t nd, double* const* L_dev,
                         const double* pred, const double* ones, const int* cmap, int64_t rows) {
    if (nd <= 0 || m <= 0) return;
    const int tiles_r = (int)((nd + 127) / 128), tiles_c = (int)(((rows > 0 ? rows : m) + 127) / 128);
    k_draw_trmm<<<dim3((unsigned)(tiles_r * tiles_c)), dim3(512), 0, s>>>(X, (long)m, E, (long)ldp, L_dev, pred, ones, cmap,
                                                                          tiles_r, tiles_c, (long)nd);
}

// srcptr_dev: readable location of every panel (== sigptr_dev in a single-process run); Jstep > 1 is the
// block-column-cyclic stride of a multi-process run
void ck_launch_syrk_group(hipStream_t s, double* const* sigptr_dev, double* const* srcptr_dev, int K0, int np, int J0,
                          int Jstep, int nJ, int64_t Npad, int64_t nvalid, unsigned long long* stamps) {
    if (nJ <= 0 || np <= 0) return;
    (void)Npad;
    const CkTileMap map = ck_tilemap_make(nvalid, J0, Jstep, nJ);
    if (map.total <= 0) return;
    const dim3 grid((unsigned)map.total);
    if (stamps)
        k_syrk_group_d<8, true><<<grid, dim3(512), 0, s>>>(sigptr_dev, srcptr_dev, K0, np, map, stamps);
    else
        k_syrk_group_d<8><<<grid, dim3(512), 0, s>>>(sigptr_dev, srcptr_dev, K0, np, map);
}

// mrows (a multiple of 128, <= mpad): only the first mrows right-hand-side rows are updated -- the leave-one-out
// sweep knows that the others are still zero in these columns
void ck_launch_aux_group(hipStream_t s, double* aux, int64_t mpad, double* const* sigptr_dev, int K0, int np, int J0,
                         int nJ, int64_t mrows, int64_t nvalid, int64_t live_rows) {
    if (nJ <= 0 || np <= 0 || mrows <= 0) return;
    const dim3 grid((unsigned)((mrows / 128) * (CK_NB / 128)), (unsigned)nJ);
    // live_rows: rows in front of the padding (m + 1; 0: all) -- a last tile row with at most 16 of them computes their block only
    const int thin_tm = live_rows > 0 && live_rows % 128 >= 1 && live_rows % 128 <= 16 ? (int)(live_rows / 128) : -1;
    k_aux_group_d<8><<<grid, dim3(512), 0, s>>>(aux, mpad, sigptr_dev, K0, np, J0, mrows, nvalid, thin_tm);
}

// plain (optionally batched over blockIdx.y) form
template <int WN>
__global__ __launch_bounds__(512, 2) void k_gemm_nt(double* __restrict__ C, long ldc, const double* __restrict__ A,
                                                     long lda, const double* __restrict__ B, long ldb, int tiles_m,
                                                     int tiles_n, int K, int lower, long diag_off, long sC, long sA,
                                                     long sB) {
    constexpr int BN = WN * 32;
    __shared__ __attribute__((aligned(16))) char lds[2 * 8 * (CK_BM + BN) * 16];
    const int t = xcd_remap(blockIdx.x, tiles_m * tiles_n);
    const int tm = t / tiles_n, tn = t - tm * tiles_n;
    const long r0 = (long)tm * CK_BM, c0 = (long)tn * BN;
    if (lower && r0 + (CK_BM - 1) + diag_off < c0) return;
    const long y = blockIdx.y;
    gemm_tile<WN>(C + y * sC, ldc, A + y * sA, lda, B + y * sB, ldb, r0, c0, K, lds);
}

// N % 128 == 0: 128 x 128 tiles (gemm_tile_e); otherwise (N a multiple of 64 only: the narrow right-hand sides of
// the panel-internal K = 64 updates) 256 x 64 tiles (gemm_tile<2>)
void ck_launch_gemm_nt(hipStream_t s, double* C, int64_t ldc, const double* A, int64_t lda, const double* B,
                       int64_t ldb, int64_t M, int64_t N, int64_t K, int lower, int64_t diag_off, int batch,
                       int64_t sC, int64_t sA, int64_t sB) {
    if (M <= 0 || N <= 0 || K <= 0 || batch <= 0) return;
    if (N % 128 == 0 && M % 128 == 0) {
        const int tm = (int)(M / 128), tn = (int)(N / 128);
        k_gemm_nt_e<<<dim3(tm * tn, batch), dim3(512), 0, s>>>(C, ldc, A, lda, B, ldb, tm, tn, (int)K, lower, diag_off,
                                                             sC, sA, sB);
        return;
    }
    const int tiles_m = (int)(M / CK_BM), tiles_n = (int)(N / 64);
    k_gemm_nt<2><<<dim3(tiles_m * tiles_n, batch), dim3(512), 0, s>>>(C, ldc, A, lda, B, ldb, tiles_m, tiles_n, (int)K,
                                                                    lower, diag_off, sC, sA, sB);
}

// ---------------------------------------------------------------------------------------
// 64 x 64 Cholesky of a diagonal block AND its inverse (one workgroup, register resident)
// ---------------------------------------------------------------------------------------
// Thread (bi, bk) = (t >> 4, t & 15) keeps the 4 x 4 block rows 4bi.., cols 4bk.. in registers.
// Right-looking on the UNSCALED columns: at step j the owners of column j publish it through a
// double-buffered LDS vector, then every thread updates a[i][k] -= a[i][j] a[k][j] / a[j][j] for
// its elements with j < k <= i.  The pivots a[j][j] are final once step j - 1 is done, so the
// scaling L[i][j] = a[i][j] / sqrt(a[j][j]) is applied once at the end.  One barrier per step,
// no LDS read-modify-write.
// Then the inverse, for the row solves against this block (k_trsm64m: a product with L^-T on the
// matrix cores instead of a 64-step substitution per row), blocked in 16 x 16 blocks (see below).
// (Measured alternatives: one wave solving X L^T = I for all 64 columns by substitution, 36 us for the
// whole kernel; carrying the inverse along inside the 64 factorisation steps -- the same row
// operations applied to an identity -- 35 us.)
// Linv: 64 x 64 row-major, lower triangle, upper zero.
// Lt, Wi: two 64 x 66 LDS arrays (Lt[c][i] = L[i][c]; Wi = the inverse, row-major) owned by the calling kernel
// PUB: what this call stores will be read by OTHER workgroups of the same launch: write-through (sc1) stores, so that the
// publisher only has to drain its stores (s_waitcnt vmcnt(0)) in front of the flag instead of writing back its XCD's L2
// (agent-scope release fence: 1.7 - 6.5 us each, MI355X_MICROARCH.md "inter-workgroup visibility")
template <bool PUB>
__device__ __forceinline__ void st_shared_result(double* p, double v) {
    if (PUB)
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        *p = v;
}

#define CK_POTRF_MARK(k)                                                            \
    if (PROF) {                                                                     \
        __syncthreads();                                                            \
        if (threadIdx.x == 0) prof[k] = (long long)__builtin_amdgcn_s_memtime();    \
    }
// PROF (diagnostic build of the kernel only: ck_debug_potrf_profile): shader-clock stamps at the phase boundaries
// COLS4: four columns per barrier (the latency-bound uses: one diagonal block at a time in the joint path's panel chain)
// or one (the local predictor's batched diagonal blocks, thousands of workgroups per launch: THROUGHPUT counts there, and
// the four-column form's redundant in-register elimination makes every workgroup do more: 10.8 -> 12.5 ms per 400 km run)
// PUB: the inverse is read by other workgroups of the same launch (k_panel_coop): write-through stores (st_shared_result)
// SRCLDS: the block to factor is handed over in Lt (LDS, row-major, pitch 66) instead of being read from A; the factor is
// still stored to A
template <bool PROF = false, bool COLS4 = true, bool PUB = false, bool SRCLDS = false>
__device__ __forceinline__ void potrf64_body(double* __restrict__ A, long ld, long g0, long long* info,
                                             double* __restrict__ Linv, double (*Lt)[66], double (*Wi)[66],
                                             long long* prof = nullptr) {
    __shared__ __attribute__((aligned(16))) double pan[2][4][68];   // the current block column, column-major (+ padding)
    __shared__ double pv[64];
    __shared__ double rdiag[64];
    double* const col0 = &pan[0][0][0];   // 64 doubles of scratch for the scaling pass below
    const int t = threadIdx.x, bi = t >> 4, bk = t & 15;
    const bool lower = bk <= bi;
    double a[4][4];
    CK_POTRF_MARK(0)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) a[r][c] = lower ? (SRCLDS ? Lt[4 * bi + r][4 * bk + c] : A[(long)(4 * bi + r) * ld + 4 * bk + c]) : 0.0;
    if (SRCLDS) __syncthreads();   // everybody holds its elements before anything is written to Lt / Wi
    if (PROF) {
        double sum = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) sum += a[r][c];
        if (sum == 1.2345e300) prof[15] = 1;   // the loads have landed
    }
    CK_POTRF_MARK(1)
    if (!COLS4) {
        // one column per barrier: at step j the owners of column j publish it through a double-buffered LDS vector, then
        // every thread updates a[i][k] -= a[i][j] a[k][j] / a[j][j] for its elements with j < k <= i
        double* const colbuf[2] = {&pan[0][0][0], &pan[1][0][0]};
        for (int jb = 0; jb < 16; ++jb) {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int j = 4 * jb + jj;
                double* cb = colbuf[jj & 1];
                if (bk == jb) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) cb[4 * bi + r] = a[r][jj];
                }
                __syncthreads();
                const double piv = cb[j];
                if (t == 0) {
                    pv[j] = piv;
                    if (!(piv > 0.0)) atomicCAS((unsigned long long*)info, 0ULL, (unsigned long long)(g0 + j + 1));
                }
                if (lower && bk >= jb) {
                    double rp = __builtin_amdgcn_rcp(piv);
                    rp = fma(fma(-piv, rp, 1.0), rp, rp);
                    rp = fma(fma(-piv, rp, 1.0), rp, rp);
                    double li[4], lk[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) li[r] = cb[4 * bi + r] * rp;
#pragma unroll
                    for (int c = 0; c < 4; ++c) lk[c] = cb[4 * bk + c];
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const bool upd = (bk > jb || c > jj) && (4 * bk + c <= 4 * bi + r);
                            if (upd) a[r][c] -= li[r] * lk[c];
                        }
                }
            }
        }
    }
    // Four columns per barrier: the owners of block column jb publish their 4 x 4 blocks (a 64 x 4 panel); every thread
    // that still has work eliminates the panel's four columns ON ITS OWN COPIES of the three pieces it needs -- the
    // 4 x 4 diagonal block D, the rows of its block row (Pi) and of its block column (Pk) -- and applies the four rank-1
    // updates to its block.  The redundant in-register elimination (48 FMAs, 4 reciprocals) costs less than the three
    // LDS round trips and barriers it replaces: 64 dependent steps become 16 (23 -> 12 us for the factorisation).
    // As before the columns stay UNSCALED (a[i][k] -= a[i][j] a[k][j] / a[j][j]); L[i][j] = a[i][j] / sqrt(a[j][j]) once
    // at the end.  Entries above the diagonal inside diagonal blocks carry garbage and are never used.
    for (int jb = 0; COLS4 && jb < 16; ++jb) {
        double (*pb)[68] = pan[jb & 1];
        if (bk == jb && bi >= jb) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                d2_t v0 = {a[0][c], a[1][c]}, v1 = {a[2][c], a[3][c]};
                *reinterpret_cast<d2_t*>(&pb[c][4 * bi]) = v0;
                *reinterpret_cast<d2_t*>(&pb[c][4 * bi + 2]) = v1;
            }
        }
        __syncthreads();
        if (lower && bk >= jb) {
            double D[4][4], Pi[4][4], Pk[4][4], rp[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const d2_t d0 = *reinterpret_cast<const d2_t*>(&pb[c][4 * jb]), d1 = *reinterpret_cast<const d2_t*>(&pb[c][4 * jb + 2]);
                const d2_t p0 = *reinterpret_cast<const d2_t*>(&pb[c][4 * bi]), p1 = *reinterpret_cast<const d2_t*>(&pb[c][4 * bi + 2]);
                const d2_t k0 = *reinterpret_cast<const d2_t*>(&pb[c][4 * bk]), k1 = *reinterpret_cast<const d2_t*>(&pb[c][4 * bk + 2]);
                D[0][c] = d0[0]; D[1][c] = d0[1]; D[2][c] = d1[0]; D[3][c] = d1[1];
                Pi[0][c] = p0[0]; Pi[1][c] = p0[1]; Pi[2][c] = p1[0]; Pi[3][c] = p1[1];
                Pk[0][c] = k0[0]; Pk[1][c] = k0[1]; Pk[2][c] = k1[0]; Pk[3][c] = k1[1];
            }
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const double piv = D[jj][jj];
                if (t == 17 * jb) {     // the diagonal block's owner records the pivots
                    pv[4 * jb + jj] = piv;
                    if (!(piv > 0.0)) atomicCAS((unsigned long long*)info, 0ULL, (unsigned long long)(g0 + 4 * jb + jj + 1));
                }
                // 1 / piv sits on the critical path: v_rcp_f64 and two Newton steps instead of the IEEE division
                double r0 = __builtin_amdgcn_rcp(piv);
                r0 = fma(fma(-piv, r0, 1.0), r0, r0);
                r0 = fma(fma(-piv, r0, 1.0), r0, r0);
                rp[jj] = r0;
#pragma unroll
                for (int c2 = jj + 1; c2 < 4; ++c2) {
                    const double f = D[c2][jj] * r0;
#pragma unroll
                    for (int r2 = c2; r2 < 4; ++r2) D[r2][c2] = fma(-D[r2][jj], f, D[r2][c2]);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        Pi[r][c2] = fma(-Pi[r][jj], f, Pi[r][c2]);
                        Pk[r][c2] = fma(-Pk[r][jj], f, Pk[r][c2]);
                    }
                }
            }
            if (bk == jb) {             // the owners' blocks ARE the panel: keep the eliminated columns
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) a[r][c] = Pi[r][c];
            } else {
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double li = Pi[r][jj] * rp[jj];
#pragma unroll
                        for (int c = 0; c < 4; ++c) a[r][c] = fma(-li, Pk[c][jj], a[r][c]);
                    }
            }
        }
    }
    CK_POTRF_MARK(2)
    __syncthreads();
    // D^-1/2 once per index (not a sqrt and a division per element)
    double* rs = col0;
    if (t < 64) {
        const double d = sqrt(pv[t]);
        rs[t] = 1.0 / d;
        rdiag[t] = 1.0 / d;           // 1 / L[t][t]
    }
    __syncthreads();
    if (lower) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int i = 4 * bi + r, k = 4 * bk + c;
                if (k <= i) {
                    const double v = (k == i) ? sqrt(pv[k]) : a[r][c] * rs[k];
                    A[(long)i * ld + k] = v;
                    Lt[k][i] = v;
                }
            }
    }
    CK_POTRF_MARK(3)
    __syncthreads();
    if (!Linv) return;   // uniform: a diagonal block with no rows below it (the last block of a local system)
    // ---- the inverse, blocked 4 x 4 in 16 x 16 blocks ----
    // A. the four diagonal blocks: wave b inverts D_b, lane r < 16 solving for column r of its inverse by
    //    right-looking substitution (16 steps, multipliers broadcast from Lt);
    // B. the blocks below the diagonal, by distance d = 1, 2, 3 from it, one wave per block on the matrix
    //    cores:  W_ij = -W_ii (sum_{k = j}^{i - 1} L_ik W_kj).  The inner sum comes out of the MFMAs in
    //    exactly the register layout the next MFMA wants for its B operand, so only finished blocks go
    //    through LDS.
    const int lane = t & 63, wv = t >> 6, li = lane & 15, g = lane >> 4;
    {
        const int o = 16 * wv;
        double x[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) x[c] = (c == li) ? 1.0 : 0.0;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            x[c] *= rdiag[o + c];
#pragma unroll
            for (int c2 = c + 1; c2 < 16; ++c2) x[c2] -= x[c] * Lt[o + c][o + c2];
        }
        if (lane < 16) {   // x[i] = D^-1[i][li]
#pragma unroll
            for (int i = 0; i < 16; ++i) Wi[o + i][o + li] = x[i];
        }
    }
    CK_POTRF_MARK(4)
    __syncthreads();
#pragma unroll
    for (int d = 1; d < 4; ++d) {
        const int i = wv + d, j = wv;            // wave wv takes block (wv + d, wv) of this level, if it exists
        if (i < 4) {
            d4_t tsum = {0.0, 0.0, 0.0, 0.0};
            for (int k = j; k < i; ++k)
#pragma unroll
                for (int s2 = 0; s2 < 4; ++s2)   // A = L_ik[row li][kk], B = W_kj[kk][col li], kk = g + 4 s2
                    tsum = __builtin_amdgcn_mfma_f64_16x16x4f64(Lt[16 * k + g + 4 * s2][16 * i + li],
                                                               Wi[16 * k + g + 4 * s2][16 * j + li], tsum, 0, 0, 0);
            d4_t w = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2)       // A = W_ii[row li][kk], B = tsum[kk][col li] = register s2 of tsum
                w = __builtin_amdgcn_mfma_f64_16x16x4f64(Wi[16 * i + li][16 * i + g + 4 * s2], tsum[s2], w, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) Wi[16 * i + g + 4 * r][16 * j + li] = -w[r];
        }
        __syncthreads();
    }
    CK_POTRF_MARK(5)
    // out: 64 x 64 row-major, the blocks above the diagonal are zero
    for (int idx = t; idx < 64 * 64; idx += 256) {
        const int r = idx >> 6, c = idx & 63;
        st_shared_result<PUB>(Linv + idx, ((c >> 4) <= (r >> 4)) ? Wi[r][c] : 0.0);
    }
    CK_POTRF_MARK(6)
}

// diagnostic: the same kernel with phase stamps (prof[0..6]: start | block loaded | factored | scaled + stored |
// inverse: diagonal blocks | inverse: off-diagonal blocks | inverse stored), shader clock
__global__ __launch_bounds__(256) void k_potrf64_prof(double* __restrict__ A, long ld, long long* info, double* __restrict__ Linv,
                                                       long long* prof) {
    __shared__ __attribute__((aligned(16))) double Lt[64][66];
    __shared__ __attribute__((aligned(16))) double Wi[64][66];
    potrf64_body<true>(A, ld, 0, info, Linv, Lt, Wi, prof);
}

void ck_launch_potrf64_prof(hipStream_t s, double* A, int64_t ld, long long* info, double* Linv, long long* prof) {
    k_potrf64_prof<<<dim3(1), dim3(256), 0, s>>>(A, ld, info, Linv, prof);
}

__global__ __launch_bounds__(256) void k_potrf64(double* __restrict__ A, long ld, long g0, long long* info,
                                                  double* __restrict__ Linv) {
    __shared__ __attribute__((aligned(16))) double Lt[64][66];
    __shared__ __attribute__((aligned(16))) double Wi[64][66];
    potrf64_body(A, ld, g0, info, Linv, Lt, Wi);
}

void ck_launch_potrf64(hipStream_t s, double* A, int64_t ld, int64_t global_index0, long long* info_dev,
                       double* Linv) {
    k_potrf64<<<dim3(1), dim3(256), 0, s>>>(A, ld, global_index0, info_dev, Linv);
}

// ---------------------------------------------------------------------------------------
// X L^T = A  (64 columns, rows independent) as  X = A Linv^T  on the matrix cores
// ---------------------------------------------------------------------------------------
// One workgroup = 64 rows, in place: the rows and Linv (k_potrf64) are staged in LDS through
// coalesced 512-byte row segments, wave w takes rows 16 w .. 16 w + 15 and the four 16-column tiles
// of X; Linv is lower triangular, so column tile jt needs k < 16 (jt + 1) only: 40 MFMA 16x16x4 per
// wave.  (The first version kept one row per lane in registers and substituted through 64 steps of
// LDS-broadcast multipliers, rows read as 512 contiguous bytes PER LANE: 27 us per launch.)
__device__ __forceinline__ void trsm64_body(double* __restrict__ A, long ld, long row0,
                                            const double* __restrict__ Linv) {
    constexpr int PITCH = 66;   // doubles per LDS row
    __shared__ __attribute__((aligned(16))) double As[64 * PITCH];
    __shared__ __attribute__((aligned(16))) double Li[64 * PITCH];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int idx = tid; idx < 64 * 64; idx += 256) {
        const int r = idx >> 6, c = idx & 63;
        As[r * PITCH + c] = A[(row0 + r) * ld + c];
        Li[r * PITCH + c] = Linv[idx];
    }
    __syncthreads();
    const int li = lane & 15, g = lane >> 4;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
        d4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4 * (jt + 1); ++s) {
            const double av = As[(16 * w + li) * PITCH + 4 * s + g];
            const double bv = Li[(16 * jt + li) * PITCH + 4 * s + g];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) A[(row0 + 16 * w + g + 4 * r) * ld + 16 * jt + li] = acc[r];
    }
}

__global__ __launch_bounds__(256, 2) void k_trsm64m(double* __restrict__ A, long ld, long nrows,
                                                     const double* __restrict__ Linv) {
    trsm64_body(A, ld, (long)blockIdx.x * 64, Linv);
}

void ck_launch_trsm64(hipStream_t s, double* A, int64_t ld, int64_t nrows, const double* Linv) {
    if (nrows <= 0) return;
    k_trsm64m<<<dim3((unsigned)(nrows / 64)), dim3(256), 0, s>>>(A, ld, nrows, Linv);   // nrows is a multiple of 64 (host)
}

// ---------------------------------------------------------------------------------------
// local-neighbourhood systems, tiled path (ck_internal.h: CkLocalSys): one 64-column step for a
// batch of independent systems, system index in blockIdx.y
// ---------------------------------------------------------------------------------------
// One 64-row chunk of block column i of the group that starts at column g0 (jb = g0 + 64 i): first the updates
// of the group's earlier blocks (left-looking inside the group),
//     C[rows, jb .. jb + 63] -= S[rows, g0 .. jb) * S[jb .. jb + 63, g0 .. jb)^T,
// then, with SOLVE, the row solve against the factored diagonal block as a product with its inverse,
//     X = C Linv^T,
// in one pass over the chunk.  K slabs of 64 columns are staged through LDS with the next slab already in
// flight in registers; the chunk of C is loaded straight into the MFMA result layout before the K loop.
// As, Bs: 64 x 66 doubles of LDS each.
// C: the chunk (64 x 64, leading dimension ld); Ar: the chunk's rows, first of the 64 i earlier columns (same ld);
// Br: the 64 rows of the block's own diagonal range, same columns (leading dimension ldb).
// COH: Br and Linv were written by OTHER workgroups of the same launch (k_panel_coop): they are read with agent-scope
// coherent loads (sc1: served from the coherence point, not from this XCD's possibly stale L2 lines)
template <bool COH>
__device__ __forceinline__ double ld_shared_result(const double* p) {
    return COH ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p;
}

// Staging (round 3, second session): the slabs arrive through buffer_load_dwordx4 -- the chunk's / the pivot's rows in a
// resource descriptor, ONE per-lane offset register (row tid >> 5 of eight, column pair tid & 31), the slab's and the row
// group's byte offset as the scalar offset (scalar adds) -- and go to LDS with ds_write_b128; the sign of A sits in the
// accumulators (-C in, negated once at the end).  Before, every one of a slab's 32 eight-byte loads per thread had its own
// 64-bit address arithmetic and every A element its own negation: ~110 vector instructions per slab and wave beside 64
// MFMAs (device assembly), and a plain vector instruction in an MFMA loop costs far more than its issue slot (gemm_tile_d).
template <bool SOLVE, bool COH = false, bool PUB = false>
__device__ __forceinline__ void lt_rows_body(double* __restrict__ C, const double* __restrict__ Ar, long ld,
                                             const double* __restrict__ Br, long ldb, int i,
                                             const double* __restrict__ Linv, double* As, double* Bs) {
    static_assert(!COH, "the coherent variant lives in k_panel_coop's own body");
    constexpr int PITCH = 66;
    typedef unsigned v4u_t __attribute__((ext_vector_type(4)));
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int srow = tid >> 5, scp = tid & 31;   // staging: elements (srow + 8 u, 2 scp .. 2 scp + 1), u < 8
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)Ar, (short)0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)Br, (short)0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsL = __builtin_amdgcn_make_buffer_rsrc((void*)Linv, (short)0, 0x7fffffff, 0x00020000);
    const int a_vo = (srow * (int)ld + 2 * scp) * 8, b_vo = (srow * (int)ldb + 2 * scp) * 8, l_vo = (srow * 64 + 2 * scp) * 8;
    const int a_rs = 8 * (int)ld * 8, b_rs = 8 * (int)ldb * 8;   // byte stride of a group of eight rows
    double* const As_w = As + srow * PITCH + 2 * scp;
    double* const Bs_w = Bs + srow * PITCH + 2 * scp;
    v4u_t ra[8], rb[8];
    if (i > 0) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            ra[u] = __builtin_amdgcn_raw_buffer_load_b128(rsA, a_vo, u * a_rs, 0);
            rb[u] = __builtin_amdgcn_raw_buffer_load_b128(rsB, b_vo, u * b_rs, 0);
        }
    }
    d4_t cn[4];   // = -(C - sum A B^T): the accumulators carry the sign, A goes to LDS as it is
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) cn[jt][r] = -C[(long)(16 * w + g + 4 * r) * ld + 16 * jt + li];
    for (int ks = 0; ks < i; ++ks) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            *reinterpret_cast<v4u_t*>(As_w + 8 * u * PITCH) = ra[u];
            *reinterpret_cast<v4u_t*>(Bs_w + 8 * u * PITCH) = rb[u];
        }
        __syncthreads();
        if (ks + 1 < i) {
            const int so = 64 * (ks + 1) * 8;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                ra[u] = __builtin_amdgcn_raw_buffer_load_b128(rsA, a_vo, so + u * a_rs, 0);
                rb[u] = __builtin_amdgcn_raw_buffer_load_b128(rsB, b_vo, so + u * b_rs, 0);
            }
        } else if (SOLVE) {
#pragma unroll
            for (int u = 0; u < 8; ++u) rb[u] = __builtin_amdgcn_raw_buffer_load_b128(rsL, l_vo, u * (8 * 64 * 8), 0);
        }
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) {
            const double av = As[(16 * w + li) * PITCH + 4 * s2 + g];
#pragma unroll
            for (int jt = 0; jt < 4; ++jt)
                cn[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Bs[(16 * jt + li) * PITCH + 4 * s2 + g], cn[jt], 0, 0, 0);
        }
        __syncthreads();
    }
    if (!SOLVE) {
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) C[(long)(16 * w + g + 4 * r) * ld + 16 * jt + li] = -cn[jt][r];
        return;
    }
    if (i == 0) {
#pragma unroll
        for (int u = 0; u < 8; ++u) rb[u] = __builtin_amdgcn_raw_buffer_load_b128(rsL, l_vo, u * (8 * 64 * 8), 0);
    }
    // the updated chunk (still negated) becomes the A operand (each wave re-reads only the 16 rows it wrote), Linv the B
    // operand; the product's sign is turned back in front of the store
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) As[(16 * w + g + 4 * r) * PITCH + 16 * jt + li] = cn[jt][r];
#pragma unroll
    for (int u = 0; u < 8; ++u) *reinterpret_cast<v4u_t*>(Bs_w + 8 * u * PITCH) = rb[u];
    __syncthreads();
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
        d4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s2 = 0; s2 < 4 * (jt + 1); ++s2)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(As[(16 * w + li) * PITCH + 4 * s2 + g],
                                                      Bs[(16 * jt + li) * PITCH + 4 * s2 + g], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) st_shared_result<PUB>(C + (long)(16 * w + g + 4 * r) * ld + 16 * jt + li, -acc[r]);
    }
}

// (Measured and removed, round 3: the same step on EIGHT waves -- 512 threads, two accumulator tiles and eight staged
// elements per thread, 122 VGPRs = four waves per SIMD instead of two -- bit-identical and no faster: local predictor at
// 400 km 99.8 -> 101.2 ms, solve sweep 219.5 -> 221.1 ms.  Two workgroups fit a CU either way (LDS), and a chunk's time is
// its chain of load -> LDS -> barrier round trips, not its MFMAs.)
// in-group update of the diagonal block itself:  D -= A A^T,  A = S[jb .. jb + 63, g0 .. jb); both operands are the
// same rows, so ONE 64 x 66 LDS array M serves as A and as B
__device__ __forceinline__ void lt_diag_update(double* __restrict__ S, long ld, int g0, int i, double* M) {
    constexpr int PITCH = 66;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, g = lane >> 4;
    const int jb = g0 + 64 * i;
    const double* Ar = S + (long)jb * ld + g0;
    double* C = S + (long)jb * ld + jb;
    const int sr = tid >> 6, sc = tid & 63;
    d4_t acc[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) acc[jt] = d4_t{0.0, 0.0, 0.0, 0.0};
    for (int ks = 0; ks < i; ++ks) {
        if (ks) __syncthreads();
#pragma unroll
        for (int u = 0; u < 16; ++u) M[(sr + 4 * u) * PITCH + sc] = Ar[(long)(sr + 4 * u) * ld + 64 * ks + sc];
        __syncthreads();
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) {
            const double av = M[(16 * w + li) * PITCH + 4 * s2 + g];
#pragma unroll
            for (int jt = 0; jt < 4; ++jt)
                acc[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, M[(16 * jt + li) * PITCH + 4 * s2 + g], acc[jt], 0, 0, 0);
        }
    }
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) C[(long)(16 * w + g + 4 * r) * ld + 16 * jt + li] -= acc[jt][r];
}

// diagonal block of block column jb = g0 + 64 i: its in-group update, then the factorisation and the inverse.
// One LDS array for everything (36 KB with the small vectors: four workgroups per CU instead of two): inside
// potrf64_body the transposed factor lives in the block-upper part (Lt[c][i], c <= i) and the inverse in the
// block-lower part (Wi[r][c], c <= r); the 16 x 16 diagonal blocks of Lt are dead once step A of the inverse has
// read them, which is when the diagonal blocks of Wi are written (same wave, program order).
__global__ __launch_bounds__(256, 3) void k_lt_potrf64(const CkLocalSys* __restrict__ sys, double* __restrict__ slab, int g0,
                                                     int i, long long* info) {
    __shared__ __attribute__((aligned(16))) double M[64][66];
    const CkLocalSys q = sys[blockIdx.x];
    double* S = slab + q.off;
    const int jb = g0 + 64 * i;
    if (i > 0) {
        lt_diag_update(S, q.ld, g0, i, &M[0][0]);
        __syncthreads();   // the block is re-read from memory by other threads of this workgroup
    }
    potrf64_body<false, false>(S + (long)jb * q.ld + jb, q.ld, jb, info + blockIdx.x,
                               jb + 64 < q.kq ? S + (long)CK_LT_ROWS(q.kq) * q.ld + (long)i * 64 * 64 : nullptr, M, M);   // inverse slot i
}

// Rows below the diagonal block of block i, INSIDE the group's diagonal region (rows < g0 + 64 gb): in-group update and
// row solve, step by step with the diagonal blocks (k_lt_potrf64) -- these few chunks are what the next diagonal block
// waits for.  The rows below the region go through all of the group's blocks at once afterwards (k_lt_rows_all).
__global__ __launch_bounds__(256, 2) void k_lt_rows(const CkLocalSys* __restrict__ sys, double* __restrict__ slab, int g0,
                                                     int i, int gb, const CkRunMap map) {
    __shared__ __attribute__((aligned(16))) double As[64 * 66];
    __shared__ __attribute__((aligned(16))) double Bs[64 * 66];
    int y, chunk;
    if (!ck_runmap_get(map, (int)blockIdx.x, y, chunk)) return;
    const CkLocalSys q = sys[y];
    const int jb = g0 + 64 * i;
    const int lim = q.kq < g0 + 64 * gb ? q.kq : g0 + 64 * gb;
    const int nchunk = (lim - jb - 64) / 64;   // rows jb + 64 .. lim - 1
    if (chunk >= nchunk) return;
    double* S = slab + q.off;
    const long row0 = jb + 64 + 64 * (long)chunk;
    lt_rows_body<true>(S + row0 * q.ld + jb, S + row0 * q.ld + g0, q.ld, S + (long)jb * q.ld + g0, q.ld, i,
                       S + (long)CK_LT_ROWS(q.kq) * q.ld + (long)i * 64 * 64, As, Bs);
}

// The rows below the group's diagonal region (row >= g0 + 64 gb): one workgroup walks a 64-row chunk through ALL of the
// group's blocks -- block i: update by the chunk's own columns of the blocks before it (still in cache: this workgroup
// wrote them), solve against diagonal block i with its inverse (slot i).  Against one launch per block over all rows
// (rounds 1-2) every chunk's columns of the group are read from memory once and written once instead of being re-read
// by every later block of the group (64 i columns at block i: 448 KB -> 256 KB per chunk and group of four), and the
// launches of a group drop from 2 gb to gb + (gb - 1) + 1, the big ones from gb to one.
__global__ __launch_bounds__(256, 2) void k_lt_rows_all(const CkLocalSys* __restrict__ sys, double* __restrict__ slab,
                                                         int g0, int gb, const CkRunMap map) {
    __shared__ __attribute__((aligned(16))) double As[64 * 66];
    __shared__ __attribute__((aligned(16))) double Bs[64 * 66];
    int y, chunk;   // one workgroup per chunk that exists (ck_tilemap.h), a system's chunks on one XCD
    if (!ck_runmap_get(map, (int)blockIdx.x, y, chunk)) return;
    const CkLocalSys q = sys[y];
    const int r_first = g0 + 64 * gb;
    const int nchunk = (q.kq - r_first) / 64;
    if (chunk >= nchunk) return;
    double* S = slab + q.off;
    const long row0 = r_first + 64 * (long)chunk;
    const double* linv = S + (long)CK_LT_ROWS(q.kq) * q.ld;
    for (int i = 0; i < gb; ++i) {
        if (i) {   // block i reads what other threads of this workgroup stored in the blocks before it
            __threadfence_block();
            __syncthreads();
        }
        const int jb = g0 + 64 * i;
        lt_rows_body<true>(S + row0 * q.ld + jb, S + row0 * q.ld + g0, q.ld, S + (long)jb * q.ld + g0, q.ld, i,
                           linv + (long)i * 64 * 64, As, Bs);
    }
}

// ---------------------------------------------------------------------------------------
// The same two kernels inside a 512-column panel of the joint factorisation (option "panel_fused"): sub-block j
// first receives the updates of the panel's earlier sub-blocks (left-looking, K = 64 j), then is factored /
// solved -- two launches per sub-block instead of three (potrf64, trsm64m, a K = 64 update of the rest of the
// panel), and every 64-column strip of the panel is read and written once instead of once per earlier sub-block.
// P: packed panel (rows x CK_NB, row 0 = the panel's own first row).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_panel_diag(double* __restrict__ P, int j, long g0, long long* info,
                                                     double* __restrict__ Linv) {
    __shared__ __attribute__((aligned(16))) double M[64][66];
    const int jb = 64 * j;
    if (j > 0) {
        lt_diag_update(P, CK_NB, 0, j, &M[0][0]);
        __syncthreads();
    }
    potrf64_body(P + (long)jb * CK_NB + jb, CK_NB, g0 + jb, info, Linv, M, M);
}

// rows below the diagonal block of sub-block j: C = X[rows, 64 j ..] (X == P for the factorisation; the
// right-hand-side rows of the solve sweep otherwise), updates from X[rows, 0 .. 64 j) and P[64 j .. 64 j + 63, 0 .. 64 j)
__global__ __launch_bounds__(256, 2) void k_panel_rows(double* X, long row_first, const double* P,
                                                        int j, const double* __restrict__ Linv) {
    __shared__ __attribute__((aligned(16))) double As[64 * 66];
    __shared__ __attribute__((aligned(16))) double Bs[64 * 66];
    const int jb = 64 * j;
    const long row0 = row_first + 64 * (long)blockIdx.x;
    lt_rows_body<true>(X + row0 * CK_NB + jb, X + row0 * CK_NB, CK_NB, P + (long)jb * CK_NB, CK_NB, j, Linv, As, Bs);
}

// all eight sub-blocks of a panel for 64 right-hand-side rows: those rows depend on nothing but the factored
// panel, so one workgroup can walk through the panel on its own (one launch per panel instead of eight).
// tail: the eight 64 x 64 inverses behind the panel's rows.
// X2 / n1: chunks n1, n1 + 1, .. are rows of a second array (the tall sweep's split panel step: the panel's rows below the head
// and the right-hand-side rows of the block column in one launch)
__global__ __launch_bounds__(256, 2) void k_panel_rows_all(double* X, const double* P, const double* tail, double* X2, int n1) {
    __shared__ __attribute__((aligned(16))) double As[64 * 66];
    __shared__ __attribute__((aligned(16))) double Bs[64 * 66];
    const int b = (int)blockIdx.x;
    double* rows = b < n1 ? X + 64L * b * CK_NB : X2 + 64L * (b - n1) * CK_NB;
    for (int j = 0; j < CK_NB / 64; ++j) {
        if (j) {   // sub-block j reads what other threads of this workgroup stored in sub-blocks < j
            __threadfence_block();
            __syncthreads();
        }
        lt_rows_body<true>(rows + 64 * j, rows, CK_NB, P + (long)(64 * j) * CK_NB, CK_NB, j, tail + (long)j * 64 * 64, As, Bs);
    }
}

// ---------------------------------------------------------------------------------------
// The whole panel step in ONE launch: k_panel_coop
// ---------------------------------------------------------------------------------------
// Workgroup b owns the 64-row chunk b of the panel and walks it left to right through the eight 64-column sub-blocks:
// sub-block j as soon as chunk j -- whose diagonal block IS the pivot block of sub-block j -- has been published
// (its rows solved, its diagonal block factored and inverted): flag[j] == seq.  The workgroups 0 .. 7 (the chunks inside
// the 512 x 512 diagonal block; dispatched first, so always resident) finish with their own diagonal block: update by
// their solved rows, potrf64_body, release fence, flag.  Everything else that 24 dependent launches per panel did --
// 8 x (64 x 64 Cholesky + inverse, row solves, K = 64 update), each waiting for the whole previous one -- happens inside
// this launch with only the true dependencies: a chunk waits for the ONE chunk above it in the chain, not for a
// grid-wide barrier.  What crosses workgroups (the pivot chunk's rows and its inverse) is STORED write-through (sc1) by the
// eight chunks of the diagonal block, drained (s_waitcnt vmcnt(0)) and announced by one lane's sc1 flag store behind a
// workgroup barrier; it is READ with sc1 loads after one lane's poll has matched and a workgroup barrier -- the hand-off
// form of MI355X_MICROARCH.md ("sc1 stores and loads on both sides"): nobody writes back or invalidates a cache (the
// first version of this kernel published with __threadfence(): ~3.5 us twice per link of the chain).  No workgroup reads
// a byte of another chunk's rows or of an inverse before its flag, so no XCD's L2 can hold an older copy of them.
// Waits are bounded (a timeout sets *err, the host then repeats the factorisation the old way).
__device__ __forceinline__ bool coop_wait(const unsigned* flag, unsigned seq, unsigned* err, unsigned spins) {
    __shared__ int ok_s;
    __syncthreads();            // the previous use of ok_s has been read by everybody
    if (threadIdx.x == 0) {
        int ok = 0;
        for (unsigned spin = 0; spin < spins; ++spin) {
            if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == seq) {
                ok = 1;
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
        if (!ok) atomicOr(err, 1u);
        ok_s = ok;
    }
    __syncthreads();
    return ok_s != 0;
}

// The two halves of lt_rows_body for the chunk that is next in the chain (its pivot block is being factored right now):
//   coop_accumulate  cn = -(C - sum_{ks < i} A_ks B_ks^T), everything that does not need the pivot block's inverse -- runs
//                    while the pivot chunk's workgroup is still inside potrf64_body;
//   coop_finish      X = -(cn Linv^T) once the inverse is published; X goes to memory AND stays in Xs (LDS, 64 x 66) for
//                    the last slab of the chunk's own diagonal update.
// Round 4: every global access of the two is a buffer instruction -- the rows in a resource descriptor (scalar registers), ONE
// per-lane offset register, the row group's and the slab's byte offset as the scalar offset -- as in lt_rows_body; what other
// workgroups of this launch wrote (pivot rows, inverse) is loaded with sc1, what they will read is stored with sc1 (the same
// cache policy as the agent-scope atomic loads / stores of round 3).  Before, each of a slab's 32 eight-byte loads per
// thread had its own 64-bit address: sixteen address pairs per operand lived in VGPRs across the K loop, the kernel sat at
// its 256-register budget with 6 of them spilled, and every reload of a spilled address carried an s_waitcnt vmcnt(0) into the
// middle of the slab's loads -- on the chain this kernel exists to shorten.  The sign sits in the accumulators (-C in,
// negated once in front of the store), so A goes to LDS as it is: sixteen v_xor per slab and thread gone as well.
#define CK_SC1 16   // cache-policy bit of the buffer builtins on gfx940+: sc1 (coherent at agent scope)
#define CK_OWN 0    // this workgroup's own rows: plain loads
typedef unsigned ck_v4u_t __attribute__((ext_vector_type(4)));
typedef unsigned ck_v2u_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t coop_rsrc(const double* p) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, (short)0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ double coop_as_double(ck_v2u_t v) {
    return __builtin_bit_cast(double, v);
}
__device__ __forceinline__ ck_v2u_t coop_as_v2u(double v) {
    return __builtin_bit_cast(ck_v2u_t, v);
}

__device__ __forceinline__ void coop_accumulate(d4_t (&cn)[4], const double* __restrict__ C, const double* __restrict__ Ar,
                                                const double* __restrict__ Br, int i, double* As, double* Bs) {
    constexpr int PITCH = 66;
    constexpr int LD = CK_NB;
    constexpr int RS = 8 * LD * 8;   // byte stride of a group of eight rows
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int srow = tid >> 5, scp = tid & 31;   // staging: elements (srow + 8 u, 2 scp .. 2 scp + 1), u < 8
    const __amdgpu_buffer_rsrc_t rsA = coop_rsrc(Ar), rsB = coop_rsrc(Br), rsC = coop_rsrc(C);
    const int s_vo = (srow * LD + 2 * scp) * 8;
    const int c_vo = ((16 * w + g) * LD + li) * 8;
    double* const As_w = As + srow * PITCH + 2 * scp;
    double* const Bs_w = Bs + srow * PITCH + 2 * scp;
    ck_v4u_t ra[8], rb[8];
    if (i > 0) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            ra[u] = __builtin_amdgcn_raw_buffer_load_b128(rsA, s_vo, u * RS, CK_OWN);     // this chunk's own earlier columns
            rb[u] = __builtin_amdgcn_raw_buffer_load_b128(rsB, s_vo, u * RS, CK_SC1);     // the pivot chunk's rows
        }
    }
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            cn[jt][r] = -coop_as_double(__builtin_amdgcn_raw_buffer_load_b64(rsC, c_vo, (4 * r * LD + 16 * jt) * 8, CK_OWN));
    for (int ks = 0; ks < i; ++ks) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            *reinterpret_cast<ck_v4u_t*>(As_w + 8 * u * PITCH) = ra[u];
            *reinterpret_cast<ck_v4u_t*>(Bs_w + 8 * u * PITCH) = rb[u];
        }
        __syncthreads();
        if (ks + 1 < i) {
            const int so = 64 * (ks + 1) * 8;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                ra[u] = __builtin_amdgcn_raw_buffer_load_b128(rsA, s_vo, so + u * RS, CK_OWN);
                rb[u] = __builtin_amdgcn_raw_buffer_load_b128(rsB, s_vo, so + u * RS, CK_SC1);
            }
        }
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) {
            const double av = As[(16 * w + li) * PITCH + 4 * s2 + g];
#pragma unroll
            for (int jt = 0; jt < 4; ++jt)
                cn[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Bs[(16 * jt + li) * PITCH + 4 * s2 + g], cn[jt], 0, 0, 0);
        }
        __syncthreads();
    }
}

template <bool PUB>
__device__ __forceinline__ void coop_finish(const d4_t (&cn)[4], double* __restrict__ C, const double* __restrict__ Linv,
                                            double* Xs, double* Bs) {
    constexpr int PITCH = 66;
    constexpr int LD = CK_NB;
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int srow = tid >> 5, scp = tid & 31;
    const __amdgpu_buffer_rsrc_t rsL = coop_rsrc(Linv), rsC = coop_rsrc(C);
    const int l_vo = (srow * 64 + 2 * scp) * 8;
    const int c_vo = ((16 * w + g) * LD + li) * 8;
    double* const Bs_w = Bs + srow * PITCH + 2 * scp;
    ck_v4u_t rl[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) rl[u] = __builtin_amdgcn_raw_buffer_load_b128(rsL, l_vo, u * (8 * 64 * 8), CK_SC1);
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) Xs[(16 * w + g + 4 * r) * PITCH + 16 * jt + li] = cn[jt][r];
#pragma unroll
    for (int u = 0; u < 8; ++u) *reinterpret_cast<ck_v4u_t*>(Bs_w + 8 * u * PITCH) = rl[u];
    __syncthreads();
    d4_t x[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
        d4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s2 = 0; s2 < 4 * (jt + 1); ++s2)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Xs[(16 * w + li) * PITCH + 4 * s2 + g], Bs[(16 * jt + li) * PITCH + 4 * s2 + g],
                                                      acc, 0, 0, 0);
        x[jt] = -acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            // (a copy first: __builtin_bit_cast applied to the vector ELEMENT x[jt][r] read element 0 for every r -- hipcc 7.2)
            const double xv = x[jt][r];
            __builtin_amdgcn_raw_buffer_store_b64(coop_as_v2u(xv), rsC, c_vo, (4 * r * LD + 16 * jt) * 8, PUB ? CK_SC1 : 0);
        }
    }
    // this wave read only its own 16 rows of Xs (LDS accesses of one wave are served in order): overwrite them with X
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) Xs[(16 * w + g + 4 * r) * PITCH + 16 * jt + li] = x[jt][r];
    __syncthreads();
}

// dacc += M M^T for the 64 x 64 slab in M (LDS, pitch 66), MFMA result layout
__device__ __forceinline__ void coop_slab_syrk(d4_t (&dacc)[4], const double* M) {
    constexpr int PITCH = 66;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, li = lane & 15, g = lane >> 4;
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2) {
        const double av = M[(16 * w + li) * PITCH + 4 * s2 + g];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
            dacc[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, M[(16 * jt + li) * PITCH + 4 * s2 + g], dacc[jt], 0, 0, 0);
    }
}

// flags: [0..7] ready (chunk b published: rows, factored diagonal block, inverse), [8..15] rows (chunk b's rows are final)
#define CK_COOP_MARK(k)                                                                      \
    if (PROF && b >= 1 && b <= 7 && threadIdx.x == 0) prof[8 * b + (k)] = (long long)__builtin_amdgcn_s_memtime();
// PROF (diagnostic instantiation, ck_debug_coop_profile): shader-clock stamps of the links 1 .. 7 -- [0] rows flag of the
// pivot chunk seen, [1] accumulation done, [2] inverse flag seen, [3] rows solved and stored, [4] drained + rows flag set,
// [5] diagonal block updated, [6] factored + inverse stored, [7] drained + flag set
// rows: the chunk's own 64 rows (ld = CK_NB) -- inside the panel for the chunks of Sigma, inside block column K of the
// right-hand-side rows for the chunks that hang below it (round 4: the forward substitution's in-panel step is the same
// walk through the eight sub-blocks, k_panel_rows_all's work as further workgroups of this launch)
template <bool PROF, bool DIAG>
__device__ __forceinline__ void panel_coop_body(double* P, double* rows, double* tail, long g0, long long* info, unsigned* flags,
                                                unsigned seq, unsigned* err, long long* prof, double* As, double* Bs,
                                                unsigned spins, int drop) {
    constexpr int NQ = CK_NB / 64;
    const int b = (int)blockIdx.x;
    const int nj = DIAG ? b : NQ;                   // sub-blocks this chunk is solved against
    constexpr bool diag = DIAG;                     // a chunk of the diagonal block: a link of the chain
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, li = lane & 15, g = lane >> 4;
    if (b == 0 && threadIdx.x == 0) __hip_atomic_store(flags + NQ, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // chunk 0 has no rows
    // Sub-block j in two halves: everything that needs only the pivot chunk's ROWS (the K loop of the update) as soon as
    // those are final -- a potrf64_body (20 us) before the pivot's inverse exists --, the product with the inverse when
    // its flag arrives.  A chunk of the diagonal block also folds the rows it has just solved into its own diagonal
    // update (from LDS), so that behind the last sub-block only one slab and the factorisation are left.
    // (the diagonal update runs on -D: dacc = -D + sum X X^T, the updated block is -dacc -- loaded here, while nothing
    // else is going on, and handed to the factorisation through LDS: no read-modify-write of D on the chain)
    d4_t dacc[4];
    {
        const __amdgpu_buffer_rsrc_t rsD = coop_rsrc(rows + 64 * (DIAG ? b : 0));
        const int d_vo = ((16 * w + g) * CK_NB + li) * 8;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                dacc[jt][r] = DIAG ? -coop_as_double(__builtin_amdgcn_raw_buffer_load_b64(rsD, d_vo, (4 * r * CK_NB + 16 * jt) * 8, 0)) : 0.0;
    }
    for (int j = 0; j < nj; ++j) {
        if (!coop_wait(flags + NQ + j, seq, err, spins)) return;      // uniform
        if (PROF && j == b - 1) CK_COOP_MARK(0)
        if (j) __threadfence_block();                     // sub-block j reads what this workgroup stored in sub-blocks < j
        __syncthreads();
        d4_t cn[4];
        coop_accumulate(cn, rows + 64 * j, rows, P + (long)(64 * j) * CK_NB, j, As, Bs);
        if (PROF && j == b - 1) CK_COOP_MARK(1)
        if (!coop_wait(flags + j, seq, err, spins)) return;
        if (PROF && j == b - 1) CK_COOP_MARK(2)
        if (diag) {
            coop_finish<true>(cn, rows + 64 * j, tail + (long)j * 64 * 64, As, Bs);
            if (PROF && j == b - 1) CK_COOP_MARK(3)
            if (j == b - 1) {
                // this chunk's rows are final (every one of them stored write-through): drain the stores, then the next link
                // may start its own accumulation
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (threadIdx.x == 0) __hip_atomic_store(flags + NQ + b, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                CK_COOP_MARK(4)
            }
            coop_slab_syrk(dacc, As);       // the rows just solved (still in LDS) into the own diagonal update
        } else {
            coop_finish<false>(cn, rows + 64 * j, tail + (long)j * 64 * 64, As, Bs);
        }
    }
    if (!diag) return;
    double* D = rows + 64 * b;
    double (*M)[66] = reinterpret_cast<double (*)[66]>(As);
    __syncthreads();                        // the last slab's reads of As are done
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) M[16 * w + g + 4 * r][16 * jt + li] = -dacc[jt][r];
    __syncthreads();
    CK_COOP_MARK(5)
    potrf64_body<false, true, true, true>(D, CK_NB, g0 + 64 * b, info, tail + (long)b * 64 * 64, M, M);
    CK_COOP_MARK(6)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the inverse (write-through stores) has left this CU
    __syncthreads();
    // drop == b (tests, option "coop_inject_panel"): this chunk never announces its block -- the waits of the chunks below
    // it must time out, set *err and leave, and the host must redo the factorisation without this kernel
    if (threadIdx.x == 0 && drop != b) __hip_atomic_store(flags + b, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    CK_COOP_MARK(7)
}

// nsig: 64-row chunks of the panel itself; workgroups nsig .. grid - 1 take the chunks of X (the right-hand-side rows of
// this block column, may be null with grid == nsig)
__global__ __launch_bounds__(256, 2) void k_panel_coop(double* P, double* tail, long g0, long long* info, unsigned* flags,
                                                        unsigned seq, unsigned* err, double* X, int nsig, unsigned spins, int drop) {
    __shared__ __attribute__((aligned(16))) double As[64 * 66];
    __shared__ __attribute__((aligned(16))) double Bs[64 * 66];
    const int b = (int)blockIdx.x;
    if (b < CK_NB / 64)
        panel_coop_body<false, true>(P, P + 64L * b * CK_NB, tail, g0, info, flags, seq, err, nullptr, As, Bs, spins, drop);
    else
        panel_coop_body<false, false>(P, b < nsig ? P + 64L * b * CK_NB : X + 64L * (b - nsig) * CK_NB, tail, g0, info, flags, seq,
                                      err, nullptr, As, Bs, spins, -1);
}

__global__ __launch_bounds__(256, 2) void k_panel_coop_prof(double* P, double* tail, long g0, long long* info, unsigned* flags,
                                                             unsigned seq, unsigned* err, long long* prof) {
    __shared__ __attribute__((aligned(16))) double As[64 * 66];
    __shared__ __attribute__((aligned(16))) double Bs[64 * 66];
    const int b = (int)blockIdx.x;
    if (b < CK_NB / 64)
        panel_coop_body<true, true>(P, P + 64L * b * CK_NB, tail, g0, info, flags, seq, err, prof, As, Bs, 2000000u, -1);
    else
        panel_coop_body<true, false>(P, P + 64L * b * CK_NB, tail, g0, info, flags, seq, err, prof, As, Bs, 2000000u, -1);
}

void ck_launch_panel_coop_prof(hipStream_t s, double* P, int64_t nrows, double* tail, int64_t g0, long long* info,
                               unsigned* flags, unsigned seq, unsigned* err, long long* prof) {
    k_panel_coop_prof<<<dim3((unsigned)(nrows / 64)), dim3(256), 0, s>>>(P, tail, (long)g0, info, flags, seq, err, prof);
}

// X / xrows: right-hand-side rows of this block column that walk through the panel in the same launch (xrows a multiple of
// 64; 0: the panel alone)
void ck_launch_panel_coop(hipStream_t s, double* P, int64_t nrows, double* tail, int64_t g0, long long* info, unsigned* flags,
                          unsigned seq, unsigned* err, double* X, int64_t xrows, unsigned spins, int drop) {
    if (nrows <= 0) return;
    if (!X) xrows = 0;
    k_panel_coop<<<dim3((unsigned)((nrows + xrows) / 64)), dim3(256), 0, s>>>(P, tail, (long)g0, info, flags, seq, err, X,
                                                                              (int)(nrows / 64), spins, drop);
}

void ck_launch_panel_rows_all(hipStream_t s, double* X, int64_t nrows, const double* P, const double* tail, double* X2,
                              int64_t nrows2) {
    if (!X2) nrows2 = 0;
    if (nrows + nrows2 <= 0) return;
    k_panel_rows_all<<<dim3((unsigned)((nrows + nrows2) / 64)), dim3(256), 0, s>>>(X, P, tail, X2, (int)(nrows / 64));
}

void ck_launch_panel_diag(hipStream_t s, double* P, int j, int64_t g0, long long* info, double* Linv) {
    k_panel_diag<<<dim3(1), dim3(256), 0, s>>>(P, j, g0, info, Linv);
}

// nrows (a multiple of 64) rows of X starting at row_first
void ck_launch_panel_rows(hipStream_t s, double* X, int64_t row_first, int64_t nrows, const double* P, int j,
                          const double* Linv) {
    if (nrows <= 0) return;
    k_panel_rows<<<dim3((unsigned)(nrows / 64)), dim3(256), 0, s>>>(X, row_first, P, j, Linv);
}

// trailing update behind a group of columns [g0, g0 + K):  C -= A A^T on 128 x 128 tiles, rows and columns
// g0 + K .. kq - 1, lower tiles only.  One workgroup per tile that exists (ck_tilemap.h: runs of systems with the same
// number of tiles); all tiles of a system run on one XCD (they share the A rows through its L2).
__global__ __launch_bounds__(512, 4) void k_lt_update(const CkLocalSys* __restrict__ sys, double* __restrict__ slab,
                                                       int g0, int K, const CkRunMap map) {
    __shared__ __attribute__((aligned(16))) char lds[2 * 256 * 128];
    int y, t;
    if (!ck_runmap_get(map, (int)blockIdx.x, y, t)) return;
    const CkLocalSys q = sys[y];
    const int o = g0 + K;
    const int T = (q.kq - o + 127) / 128;
    if (t >= T * (T + 1) / 2) return;
    int tm = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while (tm * (tm + 1) / 2 > t) --tm;
    while ((tm + 1) * (tm + 2) / 2 <= t) ++tm;
    const int tn = t - tm * (tm + 1) / 2;
    double* S = slab + q.off;
    const double* A = S + (long)o * q.ld + g0;
    gemm_tile_e<true>(S + (long)o * q.ld + o, q.ld, A, q.ld, A, q.ld, (long)tm * 128, (long)tn * 128, K, lds, q.kq - o, q.kq - o, true);
}

// LEFT-LOOKING update of a column group (round 4): before the group [g0, g0 + W) is factored, its columns -- rows g0 .. kq - 1,
// lower tiles only -- receive the updates of EVERYTHING to their left in one pass,
//     C[g0 .., g0 .. g0 + W) -= S[g0 .., 0 .. g0) * S[g0 .. g0 + W, 0 .. g0)^T        (K = g0).
// The right-looking form (k_lt_update after every group) read and wrote every trailing tile once per earlier group with K = 64 G
// = 256 -- a tile's C traffic was most of its life (0.74 of the peak); here every tile of the matrix is read and written ONCE, with
// a K loop as long as the matrix to its left.  The sequence of accumulations per element is the same (k ascending, the same
// groups of four per MFMA; the sign flips between the passes of the right-looking form were exact), so the factor keeps its bits.
__global__ __launch_bounds__(512, 4) void k_lt_left(const CkLocalSys* __restrict__ sys, double* __restrict__ slab, int g0, int W,
                                                     const CkRunMap map) {
    __shared__ __attribute__((aligned(16))) char lds[2 * 256 * 128];
    int y, t;
    if (!ck_runmap_get(map, (int)blockIdx.x, y, t)) return;
    const CkLocalSys q = sys[y];
    const int rows = q.kq - g0;                       // rows (and columns) of the trailing matrix that starts at g0
    if (rows <= 0) return;
    const int w = rows < W ? rows : W;                // the group's columns inside this system
    const int Tr = (rows + 127) / 128, Tc = (w + 127) / 128;   // Tc = 1 or 2 (W <= 256): tile (0, 1) lies above the diagonal
    const int ntile = Tr * Tc - (Tc == 2 ? 1 : 0);
    if (t >= ntile) return;
    int tm, tn;
    if (Tc == 1) {
        tm = t;
        tn = 0;
    } else if (t == 0) {
        tm = 0;
        tn = 0;
    } else {
        tm = (t + 1) >> 1;
        tn = (t + 1) & 1;
    }
    double* S = slab + q.off;
    const double* A = S + (long)g0 * q.ld;            // rows g0 .., columns 0 .. g0 - 1: both operands
    gemm_tile_e<true>(S + (long)g0 * q.ld + g0, q.ld, A, q.ld, A, q.ld, (long)tm * 128, (long)tn * 128, g0, lds, rows, w, true);
}

// the group [g0, g0 + W) of the first n_active systems (those with kq > g0): W <= 256
void ck_launch_local_tiled_left(hipStream_t s, const CkLocalSys* sys, double* slab, int n_active, int g0, int W,
                                const int* kq_host) {
    if (n_active <= 0 || g0 <= 0) return;
    const CkRunMap map = ck_runmap_make(n_active, [&](int y) {
        const int rows = kq_host[y] - g0;
        if (rows <= 0) return 0;
        const int w = rows < W ? rows : W;
        const int Tr = (rows + 127) / 128, Tc = (w + 127) / 128;
        return Tr * Tc - (Tc == 2 ? 1 : 0);
    });
    if (map.nruns == 0) return;
    k_lt_left<<<dim3((unsigned)map.off[map.nruns]), dim3(512), 0, s>>>(sys, slab, g0, W, map);
}

// block i of the group at g0 for the first n_active systems (those with kq > g0 + 64 i)
void ck_launch_local_tiled_block(hipStream_t s, const CkLocalSys* sys, double* slab, int n_active, int g0, int i,
                                 const int* kq_host, long long* info, int group_blocks) {
    if (n_active <= 0) return;
    k_lt_potrf64<<<dim3((unsigned)n_active), dim3(256), 0, s>>>(sys, slab, g0, i, info);
    const int top = g0 + 64 * group_blocks, jb = g0 + 64 * i;   // rows inside the group's diagonal region only
    const CkRunMap map = ck_runmap_make(n_active, [&](int y) { return ((kq_host[y] < top ? kq_host[y] : top) - jb - 64) / 64; });
    if (map.nruns > 0) k_lt_rows<<<dim3((unsigned)map.off[map.nruns]), dim3(256), 0, s>>>(sys, slab, g0, i, group_blocks, map);
}

void ck_launch_local_tiled_rows_all(hipStream_t s, const CkLocalSys* sys, double* slab, int n_active, int g0,
                                    int group_blocks, const int* kq_host) {
    if (n_active <= 0) return;
    const int r_first = g0 + 64 * group_blocks;
    const CkRunMap map = ck_runmap_make(n_active, [&](int y) { return (kq_host[y] - r_first) / 64; });
    if (map.nruns == 0) return;
    k_lt_rows_all<<<dim3((unsigned)map.off[map.nruns]), dim3(256), 0, s>>>(sys, slab, g0, group_blocks, map);
}

// trailing update behind the group [g0, g0 + K) for the first n_active systems (those with kq > g0 + K)
void ck_launch_local_tiled_trailing(hipStream_t s, const CkLocalSys* sys, double* slab, int n_active, int g0, int K,
                                    const int* kq_host) {
    if (n_active <= 0) return;
    const int o = g0 + K;
    const CkRunMap map = ck_runmap_make(n_active, [&](int y) {
        const int T = (kq_host[y] - o + 127) / 128;
        return T > 0 ? T * (T + 1) / 2 : 0;
    });
    if (map.nruns == 0) return;
    k_lt_update<<<dim3((unsigned)map.off[map.nruns]), dim3(512), 0, s>>>(sys, slab, g0, K, map);
}

// ---------------------------------------------------------------------------------------
// pred / pred_err reductions over the solved right-hand-side rows
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_reduce_pred(const double* __restrict__ aux, long mpad, int n_panels,
                                                      long m, long zrow, double c0, double* __restrict__ pred,
                                                      double* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= m) return;
    double s1 = 0.0, s2 = 0.0;
    for (int K = 0; K < n_panels; ++K) {
        const double* pb = aux + (long)K * mpad * CK_NB;
        const double* xr = pb + row * CK_NB;
        const double* yr = pb + zrow * CK_NB;
#pragma unroll
        for (int t = 0; t < CK_NB; t += 128) {
            const d2_t x = *reinterpret_cast<const d2_t*>(xr + t + lane * 2);
            const d2_t y = *reinterpret_cast<const d2_t*>(yr + t + lane * 2);
            s1 += x[0] * y[0] + x[1] * y[1];
            s2 += x[0] * x[0] + x[1] * x[1];
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_xor(s1, off);
        s2 += __shfl_xor(s2, off);
    }
    if (lane == 0) {
        if (c0 < 0.0) {             // raw mode (leave-one-out): V_k . y and |V_k|^2
            pred[row] = s1;
            err[row] = s2;
        } else {
            pred[row] = s1;
            double e = sqrt(c0 - s2);   // negative variance -> NaN -> 0.0 (np.nan_to_num, joint_prediction.py:78)
            err[row] = (e == e) ? e : 0.0;
        }
    }
}

// right-hand sides of the leave-one-out sweep: row 0 = the data values z, row 1 + p = unit vector of datum p of
// the withheld process (internal index g0 + p).  Row 1 + p is zero in every column before g0 + p, so the sweep
// only needs the first rows up to the current panel (ck_api.hip: aux_rows).
__global__ void k_loo_rows(double* __restrict__ aux, long mpad, long m, long g0, const double* __restrict__ z,
                           long npad, long dense) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) {   // row dense + i: unit vector of datum i (site g0 + i)
        const long g = g0 + i;
        aux[(g / CK_NB) * mpad * CK_NB + (i + dense) * CK_NB + (g % CK_NB)] = 1.0;
    }
    if (i < npad) aux[(i / CK_NB) * mpad * CK_NB + (i % CK_NB)] = z[i];   // row 0: the data values
}

// out[r] = sum_{c <= r} L[r][c] v[c] over the packed panels (simulation draw z = L eps, src/sim.py:52-54)
__global__ __launch_bounds__(256) void k_tri_matvec(double* const* __restrict__ sigptr, long npad,
                                                     const double* __restrict__ v, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= npad) return;
    const int Kr = (int)(r / CK_NB);
    double s = 0.0;
    for (int K = 0; K <= Kr; ++K) {
        const double* row = sigptr[K] + (r - (long)K * CK_NB) * CK_NB;
        const long cmax = (K == Kr) ? (r - (long)K * CK_NB) : (CK_NB - 1);
        const double* vk = v + (long)K * CK_NB;
        for (long c = lane; c <= cmax; c += 64) s += row[c] * vk[c];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) out[r] = s;
}

void ck_launch_tri_matvec(hipStream_t s, double* const* sigptr_dev, int64_t npad, const double* v, double* out) {
    k_tri_matvec<<<dim3((unsigned)((npad + 3) / 4)), dim3(256), 0, s>>>(sigptr_dev, npad, v, out);
}

void ck_launch_loo_rows(hipStream_t s, double* aux, int64_t mpad, int64_t m, int64_t g0, const double* z,
                        int64_t npad, int64_t dense) {
    const int64_t n = m > npad ? m : npad;
    k_loo_rows<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(aux, mpad, m, g0, z, npad, (long)dense);
}

void ck_launch_reduce_pred(hipStream_t s, const double* aux, int64_t mpad, int n_panels, int64_t m, int64_t zrow,
                           double c0, double* pred, double* err) {
    if (m <= 0) return;
    k_reduce_pred<<<dim3((unsigned)((m + 3) / 4)), dim3(256), 0, s>>>(aux, mpad, n_panels, m, zrow, c0, pred, err);
}

// Universal cokriging: each solved row dotted with the q = 1 + p basis rows [y; U] (the data row and the trend rows) in ONE
// pass.  A wave owns CK_UNIV_RW rows and keeps their q + 1 sums per lane in registers; the basis rows of a panel are staged
// through LDS half a panel (256 columns) at a time, so every workgroup reads them once per panel for its 4 CK_UNIV_RW rows
// instead of once per row (k_reduce_pred reads y per row).  The loads of a panel's rows are issued before the staging barrier.
// The loops over the basis rows are unrolled to CK_UNIV_QMAX with a uniform guard: the sums stay in registers.
#define CK_UNIV_RW 2
__global__ __launch_bounds__(256) void k_reduce_univ(const double* __restrict__ aux, long mpad, int n_panels, long nrows,
                                                      long brow0, int q, double* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) double ub[CK_UNIV_QMAX * 256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long row0 = (long)blockIdx.x * (4 * CK_UNIV_RW) + (long)w * CK_UNIV_RW;
    double acc[CK_UNIV_RW][CK_UNIV_QMAX + 1];
#pragma unroll
    for (int r = 0; r < CK_UNIV_RW; ++r)
#pragma unroll
        for (int j = 0; j <= CK_UNIV_QMAX; ++j) acc[r][j] = 0.0;
    for (int K = 0; K < n_panels; ++K) {
        const double* pb = aux + (long)K * mpad * CK_NB;
        d2_t x[CK_UNIV_RW][4];
#pragma unroll
        for (int r = 0; r < CK_UNIV_RW; ++r) {
            const bool live = row0 + r < nrows;
            const double* xr = pb + (live ? row0 + r : 0) * CK_NB;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                x[r][t] = *reinterpret_cast<const d2_t*>(xr + t * 128 + lane * 2);
                if (!live) x[r][t] = d2_t{0.0, 0.0};
            }
        }
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            __syncthreads();   // the previous half's basis has been read
            for (int e = threadIdx.x; e < q * 128; e += 256) {   // q rows x 256 columns, two doubles per thread and step
                const int j = e >> 7, c = (e & 127) * 2;
                *reinterpret_cast<d2_t*>(ub + j * 256 + c) =
                    *reinterpret_cast<const d2_t*>(pb + (brow0 + j) * CK_NB + hf * 256 + c);
            }
            __syncthreads();
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
                for (int r = 0; r < CK_UNIV_RW; ++r) {
                    const d2_t xv = x[r][2 * hf + tt];
                    acc[r][0] += xv[0] * xv[0] + xv[1] * xv[1];
                }
#pragma unroll
                for (int j = 0; j < CK_UNIV_QMAX; ++j) {
                    if (j < q) {
                        const d2_t bj = *reinterpret_cast<const d2_t*>(ub + j * 256 + tt * 128 + lane * 2);
#pragma unroll
                        for (int r = 0; r < CK_UNIV_RW; ++r) {
                            const d2_t xv = x[r][2 * hf + tt];
                            acc[r][1 + j] += xv[0] * bj[0] + xv[1] * bj[1];
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < CK_UNIV_RW; ++r)
#pragma unroll
        for (int j = 0; j <= CK_UNIV_QMAX; ++j) {
            if (j <= q) {
                double v = acc[r][j];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
                acc[r][j] = v;
            }
        }
    if (lane == 0)
#pragma unroll
        for (int r = 0; r < CK_UNIV_RW; ++r) {
#pragma unroll
            for (int j = 0; j <= CK_UNIV_QMAX; ++j)
                if (j <= q && row0 + r < nrows) out[(row0 + r) * (q + 1) + j] = acc[r][j];
        }
}

void ck_launch_reduce_univ(hipStream_t s, const double* aux, int64_t mpad, int n_panels, int64_t nrows, int64_t brow0, int q,
                           double* out) {
    if (nrows <= 0 || n_panels <= 0 || q < 1 || q > CK_UNIV_QMAX || brow0 < 0 || brow0 + q > mpad || nrows > mpad) return;
    const int64_t rows_per = 4 * CK_UNIV_RW;
    k_reduce_univ<<<dim3((unsigned)((nrows + rows_per - 1) / rows_per)), dim3(256), 0, s>>>(aux, (long)mpad, n_panels, (long)nrows,
                                                                                           (long)brow0, q, out);
}

// ---------------------------------------------------------------------------------------
// MFMA operand / result map probe (diagnostic)
// ---------------------------------------------------------------------------------------
__global__ void k_mfma_probe(int32_t* out) {
    const int l = threadIdx.x;
    const int i = l & 15, k = l >> 4;
    d4_t z = {0, 0, 0, 0};
    // run 1: D[i][j] = i + 1        (A[i][0] = i + 1, B[0][j] = 1)
    d4_t d1 = __builtin_amdgcn_mfma_f64_16x16x4f64(k == 0 ? (double)(i + 1) : 0.0, k == 0 ? 1.0 : 0.0, z, 0, 0, 0);
    // run 2: D[i][j] = j + 1
    d4_t d2 = __builtin_amdgcn_mfma_f64_16x16x4f64(k == 0 ? 1.0 : 0.0, k == 0 ? (double)(i + 1) : 0.0, z, 0, 0, 0);
    // run 3: both operands non-zero only at k == 2 -> 7 everywhere iff the k maps agree
    d4_t d3 = __builtin_amdgcn_mfma_f64_16x16x4f64(k == 2 ? 1.0 : 0.0, k == 2 ? 7.0 : 0.0, z, 0, 0, 0);
    for (int r = 0; r < 4; ++r) {
        out[(l * 4 + r) * 3 + 0] = (int)d1[r] - 1;
        out[(l * 4 + r) * 3 + 1] = (int)d2[r] - 1;
        out[(l * 4 + r) * 3 + 2] = (int)d3[r];
    }
}

void ck_launch_mfma_probe(hipStream_t s, int32_t* out) { k_mfma_probe<<<dim3(1), dim3(64), 0, s>>>(out); }

// FP64 MFMA issue-rate microbenchmark: `waves_per_simd` waves per SIMD, 16 independent
// accumulators each, operands in registers, no memory traffic in the loop.
template <int NACC, int WPS>
__global__ __launch_bounds__(256, WPS) void k_mfma_peak(int iters, double* sink) {
    d4_t acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = (d4_t){0.0, 0.0, 0.0, (double)i};
    // operands as in the GEMM tile: 4 A and NACC / 4 B register pairs, every MFMA a different combination
    double a[4], b[NACC / 4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = 1.0 + (threadIdx.x + 64 * i) * 1e-9;
#pragma unroll
    for (int j = 0; j < NACC / 4; ++j) b[j] = 1.0 - (threadIdx.x + 64 * j) * 1e-9;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NACC / 4; ++j)
                acc[i * (NACC / 4) + j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i * (NACC / 4) + j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(a[i]));
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    double s = 0;
#pragma unroll
    for (int i = 0; i < NACC; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (s == 12345.678) sink[0] = s;
    if (blockIdx.x == 0 && threadIdx.x == 0) {   // shader cycles and 100 MHz ticks of the loop
        sink[1] = (double)(t1 - t0);
        sink[2] = (double)(r1 - r0);
    }
}

// returns the number of MFMAs per loop iteration
int ck_launch_mfma_peak(hipStream_t s, int blocks, int waves_per_simd, int iters, double* sink) {
    if (waves_per_simd >= 4) {
        k_mfma_peak<8, 4><<<dim3(blocks), dim3(256), 0, s>>>(iters, sink);
        return 8;
    }
    if (waves_per_simd >= 2) {
        k_mfma_peak<16, 2><<<dim3(blocks), dim3(256), 0, s>>>(iters, sink);
        return 16;
    }
    k_mfma_peak<16, 1><<<dim3(blocks), dim3(256), 0, s>>>(iters, sink);
    return 16;
}

// ---------------------------------------------------------------------------------------
// where do the workgroups of a CU-masked stream run?  (ck_debug_cu_probe)
// ---------------------------------------------------------------------------------------
__global__ void k_cu_probe(unsigned* out, int spin) {
    if (threadIdx.x == 0) {
        const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_REG_HW_ID, 32 bits
        const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);   // HW_REG_XCC_ID[3:0]
        out[blockIdx.x] = (xcc << 16) | (((hw >> 13) & 7u) << 8) | (((hw >> 12) & 1u) << 4) | ((hw >> 8) & 15u);
    }
    for (int i = 0; i < spin; ++i) __builtin_amdgcn_s_sleep(64);   // keep the slot busy so that the grid spreads out
}

void ck_launch_cu_probe(hipStream_t s, unsigned* out, int n_wg, int spin) {
    k_cu_probe<<<dim3((unsigned)n_wg), dim3(64), 0, s>>>(out, spin);
}

