// The global step's second solver: A_N = M/h^2 + sum_i w_i S_i^T S_i factorised as a BLOCK-TRIDIAGONAL matrix over breadth-first
// slabs of the mesh graph (geodesic.bfs_slabs, projections.slab_plan), for meshes past the 46 000 vertices of the explicit
// inverse (asb_gstep.hip) and for a solve that costs 4 sum sp_k^2 flop per column instead of 2 N^2.
//
// In the permuted numbering A has the diagonal blocks A_kk (sp_k x sp_k) and the sparse couplings C_k = A_{k,k-1}.
//   asb_gslab_setup   S_0 = A_00, S_k = A_kk - C_k S_{k-1}^-1 C_k^T; only the explicit inverses S_k^-1 are kept, each padded to a
//                     multiple of 16 by an identity block (its inverse is that block again, exactly).  Built from the dense
//                     layer's public calls: k_gslab_scatter (a segment of the permuted CSR into a zeroed dense block),
//                     asb_gemm_nn twice (W = C_k S_{k-1}^-1, S_k -= W C_k^T) and asb_dense_spd_inverse.  A Schur complement that
//                     is not positive definite returns that call's error and leaves no solver.
//   the sweep         forward  u_k = S_k^-1 (b_k - C_k u_{k-1}),  backward  x_k = u_k - S_k^-1 (C_{k+1}^T x_{k+1}),  for all
//                     columns of the work matrix Z (Npad, Wp) at once: row = padded permuted position, Wp = W rounded up to 64
//                     and zero there.  Per slab and direction ONE k_gslab_spmm into the slab-sized scratch T (sp_max, Wp) and
//                     ONE k_gslab_gemm, in stream order; no synchronisation and no host copy sits inside a sweep.
//   k_gslab_spmm      forward T = z_k - C_k u_{k-1}, backward T = C_{k+1}^T x_{k+1}, both from ONE device CSR of the permuted A whose
//                     columns are padded row positions of Z: in a row the lower, own and upper segments are contiguous.  A block
//                     is one row x 256 columns, the lanes run along the columns, the row's entries are taken in ascending
//                     order with one FMA each.  A padding row copies its (zero) row of Z forward and is zero backward.
//   k_gslab_gemm      the hot kernel: Z_k = S_k^-1 T (forward), Z_k -= S_k^-1 T (backward), (sp x sp) (sp x Wp) with
//                     v_mfma_f64_16x16x4_f64.  A block of 4 waves owns 32 rows x 64 columns (wave w: columns 16 w .., two
//                     accumulators that share the B operand); the contraction runs in LDS stages of 16, global -> registers ->
//                     LDS, double buffered with one barrier per stage (gs_contract's scheme).  S_k^-1 is symmetric bit for bit
//                     (asb_dense_spd_inverse mirrors one triangle), so the A stage reads ROW k of it along the tile's rows: runs
//                     of 16 doubles, stored as As[k][row] with rows of 48 doubles (the k-rows of an operand fall into
//                     different bank halves); the B stage is 16 x 64 of T in rows of 80.  sp is a multiple of 16 and Wp of 64:
//                     no load carries a bounds predicate -- the only condition is block-uniform, the second 16 rows of the last
//                     row tile when sp is an odd multiple of 16.  The store is direct (k_hyper_apply's reasoning): a store
//                     instruction of a wave writes four 128-byte runs.  The contraction is NEVER split between blocks, an
//                     entry is one accumulator summed over ascending k: it does not depend on the columns around it, on the
//                     chunk or on a repeat.  No atomics.
//   k_gslab_in        frame-major (F', N, 3) -> Z through an LDS tile of 64 x 65 doubles (k_pd_transpose's rule), the rows
//                     permuted on the way: column d ld + f of row pos(v).  Z is zeroed before: padding rows and columns are zero.
//   k_gslab_rows      rows between Z and a vertex-major buffer, either way: a row is one contiguous run on both sides.  For a
//                     solve W = 3 ld with column d ld + f, so row pos(v) of Z IS rows 3 v .. 3 v + 2 of the iterate Q (3 N, ld).
// The frame-major result comes from k_pd_untranspose (asb_pdsolve.hip).
#include "asb_common.h"

#include <algorithm>
#include <cmath>
#include <vector>

typedef double gl_d4 __attribute__((ext_vector_type(4)));

#define GL_MAX_SP 8192      // the largest padded slab: three dense temporaries of that size during the set-up (1.6 GB)
#define GL_KC 16            // values of k per LDS stage of k_gslab_gemm
#define GL_TM 32            // rows per block
#define GL_TW 64            // columns per block (16 per wave)
#define GL_LDA 48           // LDS row of the A stage: 32 rows + 16
#define GL_LDB 80           // LDS row of the B stage: 64 columns + 16

struct asb_gsl {
    long long n = 0, ns = 0, npad = 0, sp_max = 0;    // vertices (0: no factor), slabs, padded rows of Z, largest padded slab
    std::vector<int> sptr, poff;                      // (ns + 1) slab boundaries in the permuted numbering; padded row offsets
    std::vector<size_t> soff;                         // (ns + 1) offsets of the S_k^-1 in Sinv
    // the permuted A: rp (n + 1) row offsets, seg (2 n) end of the lower and start of the upper segment, ci padded row positions
    int *rp = nullptr, *seg = nullptr, *ci = nullptr, *vpos = nullptr;        // vpos (n): vertex -> padded row of Z
    double *val = nullptr, *Sinv = nullptr;
    double *Z = nullptr, *T = nullptr, *V = nullptr;  // work matrix, slab scratch, vertex-major result of asb_gstep_run
};

long long asb_gslab_n(const asb_ctx* ctx) { return ctx->gsl ? ctx->gsl->n : 0; }

void asb_gslab_release(asb_ctx* ctx) {
    asb_gsl* s = ctx->gsl;
    if (!s) return;
    s->n = 0;
    (void)asb_alloc(ctx, &s->rp, 0), (void)asb_alloc(ctx, &s->seg, 0), (void)asb_alloc(ctx, &s->ci, 0), (void)asb_alloc(ctx, &s->vpos, 0);
    (void)asb_alloc(ctx, &s->val, 0), (void)asb_alloc(ctx, &s->Sinv, 0);
    (void)asb_alloc(ctx, &s->Z, 0), (void)asb_alloc(ctx, &s->T, 0), (void)asb_alloc(ctx, &s->V, 0);
}

void asb_gslab_free(asb_ctx* ctx) {               // (the buffers went with the context's registered allocations)
    delete ctx->gsl;
    ctx->gsl = nullptr;
}

// ---------------------------------------------------------------- set-up
// grid (blocks of 256 over the spr rows of the zeroed dense block D, row length ld): row r < nr gets one segment of permuted row
// p0 + r (which 0: own, 1: lower, 2: upper), its columns relative to the padded position col0; a padding row of an own
// block its 1 on the diagonal
__global__ __launch_bounds__(256) void k_gslab_scatter(const int* __restrict__ rp, const int* __restrict__ seg, const int* __restrict__ ci,
                                                       const double* __restrict__ val, int p0, int nr, int spr, int col0, int which, int ld,
                                                       double* __restrict__ D) {
    const int r = (int)blockIdx.x * 256 + threadIdx.x;
    if (r >= spr) return;
    if (r >= nr) {
        if (which == 0) D[(long long)r * ld + r] = 1.0;
        return;
    }
    const int p = p0 + r;
    const int t0 = which == 1 ? rp[p] : seg[2 * p + (which == 0 ? 0 : 1)];
    const int t1 = which == 1 ? seg[2 * p] : (which == 0 ? seg[2 * p + 1] : rp[p + 1]);
    for (int t = t0; t < t1; ++t) D[(long long)r * ld + (ci[t] - col0)] = val[t];
}

// res[p] = |sum_t A[p][c_t] y[c_t] - 1|, y = column 0 of Z, the permuted row's columns ascending
__global__ __launch_bounds__(256) void k_gslab_resid(const int* __restrict__ rp, const int* __restrict__ ci, const double* __restrict__ val,
                                                     const double* __restrict__ Z, long long Wp, int n, double* __restrict__ res) {
    const int p = (int)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    double a = 0.0;
    const int t1 = rp[p + 1];
    for (int t = rp[p]; t < t1; ++t) a = fma(val[t], Z[(long long)ci[t] * Wp], a);
    res[p] = fabs(a - 1.0);
}

// ---------------------------------------------------------------- the sweep
// grid (row tiles of 64 over rows = 3 n, frame tiles of 64): in (F, rows) frame-major -> Z[vpos[r / 3]][(r % 3) ld + f]
__global__ __launch_bounds__(256) void k_gslab_in(const double* __restrict__ in, int F, long long rows, const int* __restrict__ vpos,
                                                  double* __restrict__ Z, long long Wp, long long ld) {
    __shared__ double tile[64 * 65];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long r0 = (long long)blockIdx.x * 64;
    const int t0 = (int)blockIdx.y * 64;
    for (int fl = wv; fl < 64; fl += 4)
        if (t0 + fl < F && r0 + lane < rows) tile[fl * 65 + lane] = in[(long long)(t0 + fl) * rows + r0 + lane];
    __syncthreads();
    for (int rl = wv; rl < 64; rl += 4) {
        const long long r = r0 + rl;
        if (r < rows && t0 + lane < F) Z[(long long)vpos[r / 3] * Wp + (r % 3) * ld + t0 + lane] = tile[lane * 65 + rl];
    }
}

// grid (n, blocks of 256 over w): the first w doubles of row vpos[v] of Z <- (TO_Z) or -> row v of buf (row length ldb)
template <bool TO_Z>
__global__ __launch_bounds__(256) void k_gslab_rows(double* __restrict__ Z, long long Wp, double* __restrict__ buf, long long ldb, long long w,
                                                    const int* __restrict__ vpos) {
    const long long v = blockIdx.x, c = (long long)blockIdx.y * 256 + threadIdx.x;
    if (c >= w) return;
    double* z = Z + (long long)vpos[v] * Wp + c;
    double* b = buf + v * ldb + c;
    if (TO_Z) *z = *b;
    else *b = *z;
}

// grid (blocks of 256 over Wp, the sp padded rows of slab k); p0: its first permuted row, nr its real rows, z0 its first padded
// row.  FWD: T = z_k - C_k u_{k-1} (the lower segment); otherwise T = C_{k+1}^T x_{k+1} (the upper segment)
template <bool FWD>
__global__ __launch_bounds__(256) void k_gslab_spmm(const int* __restrict__ rp, const int* __restrict__ seg, const int* __restrict__ ci,
                                                    const double* __restrict__ val, int p0, int nr, int z0, const double* __restrict__ Z,
                                                    long long Wp, double* __restrict__ T) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    const int rl = blockIdx.y;
    if (c >= Wp) return;
    double a = FWD ? Z[(long long)(z0 + rl) * Wp + c] : 0.0;
    if (rl < nr) {                                  // the same in every lane
        const int p = p0 + rl;
        const int t0 = FWD ? rp[p] : seg[2 * p + 1], t1 = FWD ? seg[2 * p] : rp[p + 1];
        for (int t = t0; t < t1; ++t) a = fma(FWD ? -val[t] : val[t], Z[(long long)ci[t] * Wp + c], a);
    }
    T[(long long)rl * Wp + c] = a;
}

// grid (Wp / 64, row tiles of 32 over sp); Si (sp x sp) = S_k^-1, symmetric; T (sp x Wp); Zk (sp x Wp) the slab's rows of Z.
// SUB: Zk -= Si T, otherwise Zk = Si T
template <bool SUB>
__global__ __launch_bounds__(256) void k_gslab_gemm(const double* __restrict__ Si, int sp, const double* __restrict__ T, long long Wp,
                                                    double* __restrict__ Zk) {
    constexpr int A_STAGE = GL_KC * GL_LDA, B_STAGE = GL_KC * GL_LDB;
    __shared__ double As[2 * A_STAGE];
    __shared__ double Bs[2 * B_STAGE];
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long c0 = (long long)blockIdx.x * GL_TW;
    const int r0 = (int)blockIdx.y * GL_TM;
    const bool two = r0 + 16 < sp;                  // block-uniform: the tile's second 16 rows exist
    // this thread's share of a stage: A row k = tid / 16 at the tile's rows tid % 16 and 16 + tid % 16; B rows k = tid / 64 + 4 q
    const int ak = tid >> 4, ar = tid & 15, bk = tid >> 6;
    double ra0, ra1 = 0.0, rb[4];
    auto fetch = [&](int k0) {
        const double* a = Si + (long long)(k0 + ak) * sp + r0 + ar;
        ra0 = a[0];
        if (two) ra1 = a[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) rb[q] = T[(long long)(k0 + bk + 4 * q) * Wp + c0 + lane];
    };
    auto stash = [&](int buf) {
        As[buf * A_STAGE + ak * GL_LDA + ar] = ra0;
        As[buf * A_STAGE + ak * GL_LDA + 16 + ar] = ra1;
#pragma unroll
        for (int q = 0; q < 4; ++q) Bs[buf * B_STAGE + (bk + 4 * q) * GL_LDB + lane] = rb[q];
    };
    gl_d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    fetch(0);
    stash(0);
    __syncthreads();
    int cur = 0;
    for (int k0 = 0; k0 < sp; k0 += GL_KC) {
        const bool more = k0 + GL_KC < sp;
        if (more) fetch(k0 + GL_KC);
        const double* aa = As + cur * A_STAGE + i;
        const double* bb = Bs + cur * B_STAGE + wave * 16 + i;
#pragma unroll
        for (int ks = 0; ks < GL_KC / 4; ++ks) {
            const int k = ks * 4 + g;
            const double b = bb[k * GL_LDB];
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(aa[k * GL_LDA], b, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(aa[k * GL_LDA + 16], b, acc1, 0, 0, 0);
        }
        if (more) stash(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
    // accumulator q of lane (i, g): row g + 4 q of the 16, column i of the wave's 16
    double* o = Zk + (long long)(r0 + g) * Wp + c0 + wave * 16 + i;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double* at = o + (long long)(4 * q) * Wp;
        *at = SUB ? *at - acc0[q] : acc0[q];
    }
    if (two) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            double* at = o + (long long)(16 + 4 * q) * Wp;
            *at = SUB ? *at - acc1[q] : acc1[q];
        }
    }
}

// the work matrices for Wp columns
static int gsl_work(asb_ctx* ctx, asb_gsl* s, long long Wp) {
    int rc;
    if ((rc = asb_alloc(ctx, &s->Z, (size_t)s->npad * Wp))) return rc;
    return asb_alloc(ctx, &s->T, (size_t)s->sp_max * Wp);
}

// Z <- A^-1 Z in the permuted, padded numbering; Wp a multiple of 64
static void gsl_sweep(asb_ctx* ctx, const asb_gsl* s, long long Wp) {
    const unsigned gx = (unsigned)((Wp + 255) / 256), gw = (unsigned)(Wp / GL_TW);
    auto slab = [&](int k, bool fwd) {
        const int p0 = s->sptr[k], nr = s->sptr[k + 1] - p0, z0 = s->poff[k], sp = s->poff[k + 1] - z0;
        double* Zk = s->Z + (long long)z0 * Wp;
        const dim3 gs(gx, (unsigned)sp), gg(gw, (unsigned)((sp + GL_TM - 1) / GL_TM));
        if (fwd) {
            hipLaunchKernelGGL(k_gslab_spmm<true>, gs, dim3(256), 0, ctx->stream, s->rp, s->seg, s->ci, s->val, p0, nr, z0, s->Z, Wp, s->T);
            hipLaunchKernelGGL(k_gslab_gemm<false>, gg, dim3(256), 0, ctx->stream, s->Sinv + s->soff[k], sp, s->T, Wp, Zk);
        } else {
            hipLaunchKernelGGL(k_gslab_spmm<false>, gs, dim3(256), 0, ctx->stream, s->rp, s->seg, s->ci, s->val, p0, nr, z0, s->Z, Wp, s->T);
            hipLaunchKernelGGL(k_gslab_gemm<true>, gg, dim3(256), 0, ctx->stream, s->Sinv + s->soff[k], sp, s->T, Wp, Zk);
        }
    };
    for (int k = 0; k < (int)s->ns; ++k) slab(k, true);
    for (int k = (int)s->ns - 2; k >= 0; --k) slab(k, false);
}

// the rows of a vertex-major device buffer (n x w, row length ldb; n: the factor's vertices) into the zeroed Z, the sweep, and back into out (same shape)
static int gsl_solve_vm(asb_ctx* ctx, asb_gsl* s, long long n, double* buf, long long ldb, long long w, double* out, long long ldo) {
    const long long Wp = (w + 63) / 64 * 64;
    int rc;
    if ((rc = gsl_work(ctx, s, Wp))) return rc;
    ASB_HIP(ctx, hipMemsetAsync(s->Z, 0, (size_t)s->npad * Wp * sizeof(double), ctx->stream));
    const dim3 gr((unsigned)n, (unsigned)((w + 255) / 256));
    hipLaunchKernelGGL(k_gslab_rows<true>, gr, dim3(256), 0, ctx->stream, s->Z, Wp, buf, ldb, w, s->vpos);
    gsl_sweep(ctx, s, Wp);
    hipLaunchKernelGGL(k_gslab_rows<false>, gr, dim3(256), 0, ctx->stream, s->Z, Wp, out, ldo, w, s->vpos);
    ASB_CHECK_LAUNCH(ctx);
    return ASB_OK;
}

int asb_gslab_solve_fm(asb_ctx* ctx, const double* rhs, long long F, double* Qv, double* out) {
    asb_gsl* s = ctx->gsl;
    if (!s || s->n < 1) ASB_FAIL(ctx, ASB_ERR_ARG, "no slab factor on the device (asb_gslab_setup)");
    const long long n = s->n, ld = (F + 63) / 64 * 64, Wp = 3 * ld;
    int rc;
    if ((rc = gsl_work(ctx, s, Wp))) return rc;
    if (!Qv) {
        if ((rc = asb_alloc(ctx, &s->V, (size_t)3 * n * ld))) return rc;
        Qv = s->V;
    }
    ASB_HIP(ctx, hipMemsetAsync(s->Z, 0, (size_t)s->npad * Wp * sizeof(double), ctx->stream));
    hipLaunchKernelGGL(k_gslab_in, dim3((unsigned)((3 * n + 63) / 64), (unsigned)((F + 63) / 64)), dim3(256), 0, ctx->stream, rhs, (int)F, 3 * n,
                       s->vpos, s->Z, Wp, ld);
    gsl_sweep(ctx, s, Wp);
    // row pos(v) of Z is rows 3 v .. 3 v + 2 of Qv: one run of Wp doubles
    hipLaunchKernelGGL(k_gslab_rows<false>, dim3((unsigned)n, (unsigned)((Wp + 255) / 256)), dim3(256), 0, ctx->stream, s->Z, Wp, Qv, Wp, Wp, s->vpos);
    if (out) asb_pd_untranspose_launch(ctx, Qv, (int)F, 3 * n, ld, out);
    ASB_CHECK_LAUNCH(ctx);
    return ASB_OK;
}

int asb_gslab_solve_rows(asb_ctx* ctx, const double* Gt, long long rows, long long Np, double* Ot) {
    asb_gsl* s = ctx->gsl;
    if (!s || s->n < 1) ASB_FAIL(ctx, ASB_ERR_ARG, "no slab factor on the device (asb_gslab_setup)");
    asb_tmp<double> tmp;                            // (Np, rows): the vertices' rows, the columns of the solve contiguous
    int rc;
    if ((rc = tmp.alloc(ctx, (size_t)Np * rows))) return rc;
    if ((rc = asb_transpose(ctx, Gt, rows, Np, tmp.get()))) return rc;
    if ((rc = gsl_solve_vm(ctx, s, s->n, tmp.get(), rows, rows, tmp.get(), rows))) return rc;
    return asb_transpose(ctx, tmp.get(), Np, rows, Ot);
}

extern "C" int asb_gslab_setup(asb_ctx* ctx, int64_t n, const int64_t* indptr, const int64_t* indices, const double* data, int64_t nslab,
                               const int64_t* slab_ptr, const int64_t* order, double* resid_out) {
    if (!ctx || !indptr || !slab_ptr || !order || n < 1 || nslab < 1) return ASB_ERR_ARG;
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    // the context holds one solver: the explicit inverse goes, and an earlier factor
    ctx->gs_n = 0;
    asb_rf_invalidate_all(ctx);
    (void)asb_alloc(ctx, &ctx->gs_Ainv, 0);
    asb_gslab_release(ctx);
    asb_gsub_release(ctx);
    if (nslab > n) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_gslab_setup: %lld slabs for %lld vertices", (long long)nslab, (long long)n);
    if (n + 16 * nslab > 0x7fffffffLL)
        ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_gslab_setup: %lld vertices in %lld slabs: the padded rows do not fit 32-bit indices", (long long)n, (long long)nslab);
    std::vector<int> p32, c32;
    int rc;
    if ((rc = asb_gs_check_matrix(ctx, "asb_gslab_setup", n, indptr, indices, data, p32, c32))) return rc;
    // ---- the slabs cover 0 .. n, order is a permutation, A is block tridiagonal over the slabs
    if (slab_ptr[0] != 0 || slab_ptr[nslab] != n)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_gslab_setup: the slabs run from %lld to %lld: they do not cover 0 .. %lld", (long long)slab_ptr[0],
                 (long long)slab_ptr[nslab], (long long)n);
    const int ns = (int)nslab;
    std::vector<int> sptr((size_t)ns + 1), poff((size_t)ns + 1, 0);
    std::vector<size_t> soff((size_t)ns + 1, 0);
    long long sp_max = 0;
    for (int k = 0; k < ns; ++k) {
        if (slab_ptr[k + 1] <= slab_ptr[k] || slab_ptr[k + 1] > n)
            ASB_FAIL(ctx, ASB_ERR_ARG, "asb_gslab_setup: slab %d runs from %lld to %lld: they do not cover 0 .. %lld in ascending order", k,
                     (long long)slab_ptr[k], (long long)slab_ptr[k + 1], (long long)n);
        const long long sp = (slab_ptr[k + 1] - slab_ptr[k] + 15) / 16 * 16;
        if (sp > GL_MAX_SP)
            ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_gslab_setup: slab %d has %lld vertices (at most %d): choose a smaller slab_target", k,
                     (long long)(slab_ptr[k + 1] - slab_ptr[k]), GL_MAX_SP);
        sp_max = std::max(sp_max, sp);
        sptr[k] = (int)slab_ptr[k], poff[k + 1] = poff[k] + (int)sp, soff[k + 1] = soff[k] + (size_t)sp * sp;
    }
    sptr[ns] = (int)n;
    std::vector<int> inv((size_t)n, -1), slab_of((size_t)n);     // vertex -> permuted index; permuted index -> slab
    for (int64_t p = 0; p < n; ++p) {
        const int64_t v = order[p];
        if (v < 0 || v >= n || inv[v] >= 0)
            ASB_FAIL(ctx, ASB_ERR_ARG, "asb_gslab_setup: order[%lld] = %lld: not a permutation of 0 .. %lld", (long long)p, (long long)v, (long long)n - 1);
        inv[v] = (int)p;
    }
    for (int k = 0; k < ns; ++k)
        for (int p = sptr[k]; p < sptr[k + 1]; ++p) slab_of[p] = k;
    const int64_t nnz = indptr[n];
    // ---- the permuted CSR, its columns as padded rows of Z and ascending
    std::vector<int> rp((size_t)n + 1, 0), seg((size_t)2 * n), ci((size_t)nnz + 1), vpos((size_t)n);
    std::vector<double> val((size_t)nnz + 1);
    std::vector<std::pair<int, double>> row;
    for (int64_t p = 0; p < n; ++p) {
        const int64_t v = order[p];
        const int k = slab_of[p];
        vpos[v] = poff[k] + (int)(p - sptr[k]);
        row.clear();
        for (int64_t t = indptr[v]; t < indptr[v + 1]; ++t) {
            const int q = inv[indices[t]], kq = slab_of[q];
            if (kq < k - 1 || kq > k + 1)
                ASB_FAIL(ctx, ASB_ERR_ARG, "asb_gslab_setup: entry (%lld, %lld) couples slabs %d and %d: the matrix is not block tridiagonal over the slabs",
                         (long long)v, (long long)indices[t], k, kq);
            row.emplace_back(poff[kq] + (q - sptr[kq]), data[t]);
        }
        std::sort(row.begin(), row.end());
        int at = rp[p], lo_end = at, up_begin = at;
        for (const auto& e : row) {
            ci[at] = e.first, val[at] = e.second;
            if (e.first < poff[k]) lo_end = at + 1;
            if (e.first < poff[k + 1]) up_begin = at + 1;
            ++at;
        }
        seg[2 * p] = lo_end, seg[2 * p + 1] = up_begin, rp[p + 1] = at;
    }
    if (!ctx->gsl) ctx->gsl = new asb_gsl();
    asb_gsl* s = ctx->gsl;
    s->ns = ns, s->npad = poff[ns], s->sp_max = sp_max, s->sptr = sptr, s->poff = poff, s->soff = soff;
    if ((rc = asb_alloc(ctx, &s->rp, rp.size()))) return rc;
    if ((rc = asb_alloc(ctx, &s->seg, seg.size()))) return rc;
    if ((rc = asb_alloc(ctx, &s->ci, ci.size()))) return rc;
    if ((rc = asb_alloc(ctx, &s->val, val.size()))) return rc;
    if ((rc = asb_alloc(ctx, &s->vpos, vpos.size()))) return rc;
    if ((rc = asb_alloc(ctx, &s->Sinv, soff[ns]))) return rc;
    asb_tmp<double> Cd, Ct, Wm, dy;
    if (ns > 1) {
        if ((rc = Cd.alloc(ctx, (size_t)sp_max * sp_max))) return rc;
        if ((rc = Ct.alloc(ctx, (size_t)sp_max * sp_max))) return rc;
        if ((rc = Wm.alloc(ctx, (size_t)sp_max * sp_max))) return rc;
    }
    if ((rc = dy.alloc(ctx, (size_t)2 * n))) return rc;
    ASB_HIP(ctx, hipMemcpyAsync(s->rp, rp.data(), rp.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemcpyAsync(s->seg, seg.data(), seg.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemcpyAsync(s->ci, ci.data(), ci.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemcpyAsync(s->val, val.data(), val.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemcpyAsync(s->vpos, vpos.data(), vpos.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemsetAsync(s->Sinv, 0, soff[ns] * sizeof(double), ctx->stream));
    for (int k = 0; k < ns; ++k) {
        const int p0 = sptr[k], nr = sptr[k + 1] - p0, sp = poff[k + 1] - poff[k];
        double* S = s->Sinv + soff[k];
        const unsigned gr = (unsigned)((sp + 255) / 256);
        hipLaunchKernelGGL(k_gslab_scatter, dim3(gr), dim3(256), 0, ctx->stream, s->rp, s->seg, s->ci, s->val, p0, nr, sp, poff[k], 0, sp, S);
        if (k > 0) {                                // S_k = A_kk - (C_k S_{k-1}^-1) C_k^T, C_k^T taken from the rows of slab k - 1
            const int q0 = sptr[k - 1], nq = sptr[k] - q0, sq = poff[k] - poff[k - 1];
            ASB_HIP(ctx, hipMemsetAsync(Cd.get(), 0, (size_t)sp * sq * sizeof(double), ctx->stream));
            ASB_HIP(ctx, hipMemsetAsync(Ct.get(), 0, (size_t)sp * sq * sizeof(double), ctx->stream));
            hipLaunchKernelGGL(k_gslab_scatter, dim3(gr), dim3(256), 0, ctx->stream, s->rp, s->seg, s->ci, s->val, p0, nr, sp, poff[k - 1], 1, sq,
                               Cd.get());
            hipLaunchKernelGGL(k_gslab_scatter, dim3((unsigned)((sq + 255) / 256)), dim3(256), 0, ctx->stream, s->rp, s->seg, s->ci, s->val, q0, nq,
                               sq, poff[k], 2, sp, Ct.get());
            ASB_CHECK_LAUNCH(ctx);
            if ((rc = asb_gemm_nn(ctx, Cd.get(), sq, s->Sinv + soff[k - 1], sq, Wm.get(), sq, sp, sq, sq, 1.0, 0.0))) return rc;
            if ((rc = asb_gemm_nn(ctx, Wm.get(), sq, Ct.get(), sp, S, sp, sp, sp, sq, -1.0, 1.0))) return rc;
        }
        ASB_CHECK_LAUNCH(ctx);
        if ((rc = asb_dense_spd_inverse(ctx, S, sp))) return rc;      // (drains the stream: the staging vectors may go after the first)
    }
    // ---- resid = max |A (A^-1 1) - 1| through the sweep and the sparse A
    std::vector<double> res((size_t)n, 1.0);
    ASB_HIP(ctx, hipMemcpyAsync(dy.get(), res.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = gsl_solve_vm(ctx, s, n, dy.get(), 1, 1, dy.get(), 1))) return rc;
    hipLaunchKernelGGL(k_gslab_resid, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, s->rp, s->ci, s->val, s->Z, 64LL, (int)n,
                       dy.get() + n);
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipMemcpyAsync(res.data(), dy.get() + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));          // the staging vectors and the temporaries die here
    double worst = 0.0;
    for (int64_t i = 0; i < n; ++i) worst = (res[i] > worst || res[i] != res[i]) ? res[i] : worst;
    if (resid_out) *resid_out = worst;
    s->n = n;
    return ASB_OK;
}

// test hook: out_host (n, w) = A^-1 rhs_host (n, w) through the sweep, any w >= 1
extern "C" int asb_test_gslab_solve(asb_ctx* ctx, const double* rhs_host, int64_t w, double* out_host) {
    if (!ctx || !rhs_host || !out_host || w < 1) return ASB_ERR_ARG;
    asb_gsl* s = ctx->gsl;
    if (!s || s->n < 1) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_test_gslab_solve: no slab factor on the device (asb_gslab_setup)");
    if (w > (1 << 24)) ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_test_gslab_solve: %lld columns", (long long)w);
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    asb_tmp<double> d;
    int rc = asb_test_stage(ctx, rhs_host, (size_t)s->n * w, 0, d);
    if (!rc) rc = gsl_solve_vm(ctx, s, s->n, d.get(), w, w, d.get(), w);
    return asb_test_finish(ctx, rc, d.get(), out_host, (size_t)s->n * w);
}

// timing hook (tools/time_gslab.py): ms_out (2) = the best of three of k_gslab_gemm and of asb_gemm_nn on the same product
// (sp x sp) (sp x w) of zero-filled device buffers, device events around each; sp a multiple of 16, w of 64
extern "C" int asb_test_gslab_gemm_time(asb_ctx* ctx, int64_t sp, int64_t w, double* ms_out) {
    if (!ctx || !ms_out || sp < 16 || (sp & 15) || sp > GL_MAX_SP || w < 64 || (w & 63) || w > (1 << 24)) return ASB_ERR_ARG;
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    asb_tmp<double> Si, T, Z;
    int rc;
    if ((rc = Si.alloc(ctx, (size_t)sp * sp)) || (rc = T.alloc(ctx, (size_t)sp * w)) || (rc = Z.alloc(ctx, (size_t)sp * w))) return rc;
    ASB_HIP(ctx, hipMemsetAsync(Si.get(), 0, (size_t)sp * sp * sizeof(double), ctx->stream));
    ASB_HIP(ctx, hipMemsetAsync(T.get(), 0, (size_t)sp * w * sizeof(double), ctx->stream));
    hipEvent_t e0, e1;
    ASB_HIP(ctx, hipEventCreate(&e0));
    ASB_HIP(ctx, hipEventCreate(&e1));
    for (int which = 0; which < 2 && !rc; ++which) {
        float best = 1e30f;
        for (int rep = 0; rep < 4 && !rc; ++rep) {               // (the first run warms up and is not counted)
            (void)hipEventRecord(e0, ctx->stream);
            if (which == 0)
                hipLaunchKernelGGL(k_gslab_gemm<false>, dim3((unsigned)(w / GL_TW), (unsigned)((sp + GL_TM - 1) / GL_TM)), dim3(256), 0, ctx->stream,
                                   Si.get(), (int)sp, T.get(), (long long)w, Z.get());
            else
                rc = asb_gemm_nn(ctx, Si.get(), sp, T.get(), w, Z.get(), w, (int)sp, (int)w, (int)sp, 1.0, 0.0);
            (void)hipEventRecord(e1, ctx->stream);
            (void)hipEventSynchronize(e1);
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, e0, e1);
            if (rep > 0 && ms < best) best = ms;
        }
        ms_out[which] = best;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return rc;
    ASB_CHECK_LAUNCH(ctx);
    return ASB_OK;
}

// what the set-up left: counts_out (4) = slabs, largest padded slab, padded rows, doubles of the factor
extern "C" int asb_gslab_info(asb_ctx* ctx, int64_t* counts_out) {
    if (!ctx || !counts_out) return ASB_ERR_ARG;
    const asb_gsl* s = ctx->gsl;
    if (!s || s->n < 1) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_gslab_info: no slab factor on the device (asb_gslab_setup)");
    counts_out[0] = s->ns, counts_out[1] = s->sp_max, counts_out[2] = s->npad, counts_out[3] = (int64_t)s->soff[(size_t)s->ns];
    return ASB_OK;
}
