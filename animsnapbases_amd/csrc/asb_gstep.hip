// Global step of projective dynamics on the resident animation: q = A^-1 (b + M/h^2 s), A = M/h^2 + sum_i w_i S_i^T S_i
// (projective_dynamics/Simulators.py:117-145 prepare_global_matrix, :494-526 step), for a batch of frames at once.
//
// The reference's 3N x 3N system matrix is kron(A_N, I_3): one N x N matrix serves the three coordinates, and a right-hand side
// (F', N, 3) is F' x 3 right-hand sides of it.  With thousands of frames against one matrix the explicit inverse pays:
//
//   asb_gstep_setup    once per (constraints, masses, h): the host CSR of A_N is checked (symmetric pattern and values, positive
//                      diagonal), scattered into a dense Np x Np matrix (Np = N rounded up to 32, the padding an identity block:
//                      its inverse is that block again, exactly) and inverted in place by asb_dense_spd_inverse.  A^-1 belongs
//                      to the context.  The residual max |A (A^-1 u) - u|, u = 1, comes from the SPARSE A: k_gs_colsum sums
//                      column m of A^-1 over ascending rows (what the product kernel does with rhs = u), k_gs_resid walks row
//                      i of A in ascending column order.
//   asb_gstep_run      out[f, m, d] = sum_n rhs[f, n, d] A^-1[n, m] on frame-major (F', N, 3) tensors, neither transposed.
//                      k_gstep_gemm: v_mfma_f64_16x16x4_f64 with frames on the accumulator rows (A operand = rhs, B = A^-1), a
//                      block of 4 waves owns 64 frames x 32 vertices x 3 coordinates, so the three coordinates share every tile
//                      of A^-1.  The contraction runs in LDS stages of 16 values of n, global -> registers -> LDS, double
//                      buffered with one barrier per stage: per stage 64 frames x 48 contiguous doubles of rhs and 16 x 32 of
//                      A^-1; loads past N or past F' are zero-filled and never leave the buffers.  Epilogue as k_rforce_gemm:
//                      LDS rows of 97 doubles (the operand buffers are dead by then and are reused), 96 contiguous doubles per
//                      frame.  The contraction is never split: entry (f, m, d) is ONE accumulator summed over ascending n,
//                      whatever tile it falls in, so repeats and frame sub-ranges give identical bits.  No atomics.  The
//                      tile's loop and epilogue live in asb_gstep_tile.h, shared with k_pdsolve_gemm (asb_pdsolve.hip).
//   asb_gstep_inertia  rhs[f, n, d] += diag[n] s_f[n, d], the inertia term M/h^2 s of the selected frames, from the world
//                      positions of asb_cproj.hip (cp_pos: same reciprocals, training or held-out tensor).  Elementwise; a block
//                      of GS_VB vertices x 64 frames reads the vertex-major tensor along the frames and stages through LDS to
//                      write per frame its contiguous run, a read-modify-write of its own entries.  k_gs_inertia<false>
//                      stores the same values instead of adding them (asb_gs_inertia_launch, for asb_pdsolve_begin).
// The context holds this inverse OR the block-tridiagonal slab factor of asb_gslab.hip (each set-up releases the other): with the
// factor held asb_gstep_run goes through its sweep and asb_test_gstep_inverse is refused; with the inverse held nothing changed.
// The third holder is the position subspace of asb_gsub.hip: asb_gstep_run then applies its affine map o' + P rhs.
#include "asb_gstep_tile.h"

#include <algorithm>
#include <cmath>
#include <vector>

#define GS_MAX_N 46000      // the limit of the dense geodesics: Np^2 doubles = 17 GB
#define GS_VB 16            // vertices per block of k_gs_inertia

// ---------------------------------------------------------------- set-up
// grid (blocks over Np rows): row r of the zeroed dense matrix gets its CSR entries; a padding row its 1 on the diagonal
__global__ __launch_bounds__(256) void k_gs_fill(const int* __restrict__ ptr, const int* __restrict__ ci, const double* __restrict__ val,
                                                 int n, int np, double* __restrict__ M) {
    const int r = (int)blockIdx.x * 256 + threadIdx.x;
    if (r >= np) return;
    if (r >= n) {
        M[(long long)r * np + r] = 1.0;
        return;
    }
    const int t1 = ptr[r + 1];
    for (int t = ptr[r]; t < t1; ++t) M[(long long)r * np + ci[t]] = val[t];
}

// y[m] = sum_n Ainv[n][m], n ascending over the n real rows: the product of k_gstep_gemm for rhs = 1
__global__ __launch_bounds__(256) void k_gs_colsum(const double* __restrict__ Ainv, int n, int np, double* __restrict__ y) {
    const int m = (int)blockIdx.x * 256 + threadIdx.x;
    if (m >= n) return;
    double a = 0.0;
    for (int r = 0; r < n; ++r) a += Ainv[(long long)r * np + m];
    y[m] = a;
}

// res[i] = |sum_t A[i][c_t] y[c_t] - 1|, the row's columns ascending
__global__ __launch_bounds__(256) void k_gs_resid(const int* __restrict__ ptr, const int* __restrict__ ci, const double* __restrict__ val,
                                                  const double* __restrict__ y, int n, double* __restrict__ res) {
    const int i = (int)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double a = 0.0;
    const int t1 = ptr[i + 1];
    for (int t = ptr[i]; t < t1; ++t) a = fma(val[t], y[ci[t]], a);
    res[i] = fabs(a - 1.0);
}

int asb_gs_check_matrix(asb_ctx* ctx, const char* who, int64_t n, const int64_t* indptr, const int64_t* indices, const double* data,
                        std::vector<int>& p32, std::vector<int>& c32) {
    if (!ctx->X || ctx->v0 != 0 || ctx->n_loc != ctx->N_glob) ASB_FAIL(ctx, ASB_ERR_ARG, "%s: no whole tensor on the device (one rank only)", who);
    if (n != ctx->n_loc)
        ASB_FAIL(ctx, ASB_ERR_ARG, "%s: the matrix has %lld rows, the tensor %lld vertices", who, (long long)n, (long long)ctx->n_loc);
    int rc;
    if ((rc = asb_csr_check32(ctx, who, n, indptr, indices, data, n, p32, c32, "the system matrix"))) return rc;
    // ---- finite values, positive diagonal, symmetric pattern, symmetric values to 1e-12 of the row's largest entry
    std::vector<double> rmax((size_t)n, 0.0);
    for (int64_t i = 0; i < n; ++i) {
        double dg = 0.0;
        for (int64_t t = indptr[i]; t < indptr[i + 1]; ++t) {
            if (!std::isfinite(data[t])) ASB_FAIL(ctx, ASB_ERR_ARG, "%s: row %lld holds a value that is not finite", who, (long long)i);
            if (indices[t] == i) dg = data[t];
            if (std::fabs(data[t]) > rmax[i]) rmax[i] = std::fabs(data[t]);
        }
        if (!(dg > 0.0)) ASB_FAIL(ctx, ASB_ERR_ARG, "%s: the diagonal of row %lld is %g (must be positive)", who, (long long)i, dg);
    }
    for (int64_t i = 0; i < n; ++i)
        for (int64_t t = indptr[i]; t < indptr[i + 1]; ++t) {
            const int64_t j = indices[t];
            if (j == i) continue;
            const int* lo = c32.data() + indptr[j];
            const int* hi = c32.data() + indptr[j + 1];
            const int* at = std::lower_bound(lo, hi, (int)i);
            if (at == hi || *at != (int)i)
                ASB_FAIL(ctx, ASB_ERR_ARG, "%s: entry (%lld, %lld) has no mirror: the pattern is not symmetric", who, (long long)i, (long long)j);
            const double other = data[at - c32.data()];
            if (std::fabs(data[t] - other) > 1e-12 * rmax[i])
                ASB_FAIL(ctx, ASB_ERR_ARG, "%s: entries (%lld, %lld) = %.17g and its mirror %.17g differ: not symmetric", who, (long long)i,
                         (long long)j, data[t], other);
        }
    return ASB_OK;
}

extern "C" int asb_gstep_setup(asb_ctx* ctx, int64_t n, const int64_t* indptr, const int64_t* indices, const double* data, double* resid_out) {
    if (!ctx || !indptr || n < 1) return ASB_ERR_ARG;
    ctx->gs_n = 0;
    asb_rf_invalidate_all(ctx);
    asb_gslab_release(ctx);                                   // the context holds one solver
    asb_gsub_release(ctx);
    if (n > GS_MAX_N)
        ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_gstep_setup: %lld vertices are too many for an explicit inverse (at most %d)", (long long)n, GS_MAX_N);
    std::vector<int> p32, c32;
    int rc;
    if ((rc = asb_gs_check_matrix(ctx, "asb_gstep_setup", n, indptr, indices, data, p32, c32))) return rc;
    const int ni = (int)n, np = (ni + GS_TN - 1) / GS_TN * GS_TN;
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    asb_tmp<int> dptr, dci;
    asb_tmp<double> dval, dy;
    if ((rc = dptr.alloc(ctx, p32.size()))) return rc;
    if ((rc = dci.alloc(ctx, c32.size() + 1))) return rc;
    if ((rc = dval.alloc(ctx, c32.size() + 1))) return rc;
    if ((rc = dy.alloc(ctx, (size_t)2 * n))) return rc;
    if ((rc = asb_alloc(ctx, &ctx->gs_Ainv, (size_t)np * np))) return rc;
    if ((rc = asb_csr_stage(ctx, p32, c32, data, dptr.get(), dci.get(), dval.get()))) return rc;
    ASB_HIP(ctx, hipMemsetAsync(ctx->gs_Ainv, 0, (size_t)np * np * sizeof(double), ctx->stream));
    hipLaunchKernelGGL(k_gs_fill, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, ctx->stream, dptr.get(), dci.get(), dval.get(), ni, np,
                       ctx->gs_Ainv);
    ASB_CHECK_LAUNCH(ctx);
    if ((rc = asb_dense_spd_inverse(ctx, ctx->gs_Ainv, np))) return rc;
    const unsigned gr = (unsigned)((ni + 255) / 256);
    hipLaunchKernelGGL(k_gs_colsum, dim3(gr), dim3(256), 0, ctx->stream, ctx->gs_Ainv, ni, np, dy.get());
    hipLaunchKernelGGL(k_gs_resid, dim3(gr), dim3(256), 0, ctx->stream, dptr.get(), dci.get(), dval.get(), dy.get(), ni, dy.get() + n);
    ASB_CHECK_LAUNCH(ctx);
    std::vector<double> res((size_t)n);
    ASB_HIP(ctx, hipMemcpyAsync(res.data(), dy.get() + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));          // the staging vectors and the temporaries die here
    double worst = 0.0;
    for (int64_t i = 0; i < n; ++i) worst = (res[i] > worst || res[i] != res[i]) ? res[i] : worst;
    if (resid_out) *resid_out = worst;
    ctx->gs_n = n, ctx->gs_Np = np;
    return ASB_OK;
}

// ---------------------------------------------------------------- the product
// grid (Np / GS_TN, frame tiles); rhs and out (F, n, 3) frame-major; Ainv (np x np), only its n x n block is read.  The tile's
// loop and epilogue: asb_gstep_tile.h
__global__ __launch_bounds__(256) void k_gstep_gemm(const double* __restrict__ rhs, const double* __restrict__ Ainv, int n, int np,
                                                    long long F, double* __restrict__ out) {
    __shared__ double sm[GS_SM];
    const int m0 = (int)blockIdx.x * GS_TN;
    const long long t0 = (long long)blockIdx.y * GS_TF;
    d4 acc[3][2];
    gs_contract(rhs, Ainv, n, np, F, m0, t0, sm, acc);
    gs_store_fm(acc, sm, n, F, m0, t0, out);
}

extern "C" int asb_gstep_run(asb_ctx* ctx, const double* rhs_dev, int64_t n_frames, double* out_dev) {
    if (!ctx || !rhs_dev || !out_dev) return ASB_ERR_ARG;
    const long long n_sub = asb_gsub_n(ctx);
    const long long n_slab = n_sub > 0 ? n_sub : asb_gslab_n(ctx);    // (either: the vertices of the solver that is no inverse)
    if (n_slab < 1 && (ctx->gs_n < 1 || !ctx->gs_Ainv)) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_gstep_run: no inverse on the device (asb_gstep_setup)");
    if (n_frames < 1 || (n_frames + GS_TF - 1) / GS_TF > 65535)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_gstep_run: %lld frames in one call (1 .. %d)", (long long)n_frames, 65535 * GS_TF);
    const long long len = (long long)n_frames * (n_slab > 0 ? n_slab : ctx->gs_n) * 3;
    if (rhs_dev < out_dev + len && out_dev < rhs_dev + len)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_gstep_run: the right-hand side and the output overlap (the product is not done in place)");
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    if (n_sub > 0) {                                          // the position subspace: in -> reduce -> expand, frame-major too
        int rc;
        if ((rc = asb_gsub_solve_fm(ctx, rhs_dev, n_frames, nullptr, out_dev))) return rc;
        ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return ASB_OK;
    }
    if (n_slab > 0) {                                         // the slab factor: in -> sweep -> rows -> k_pd_untranspose
        int rc;
        if ((rc = asb_gslab_solve_fm(ctx, rhs_dev, n_frames, nullptr, out_dev))) return rc;
        ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return ASB_OK;
    }
    const dim3 grid((unsigned)(ctx->gs_Np / GS_TN), (unsigned)((n_frames + GS_TF - 1) / GS_TF));
    hipLaunchKernelGGL(k_gstep_gemm, grid, dim3(256), 0, ctx->stream, rhs_dev, ctx->gs_Ainv, (int)ctx->gs_n, (int)ctx->gs_Np,
                       (long long)n_frames, out_dev);
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));          // the caller owns out_dev and may read it on any stream
    return ASB_OK;
}

// ---------------------------------------------------------------- the inertia term
// grid (vertex blocks, frame tiles); rhs (n_sel, n_verts, 3).  mode 0: s = x_f + acc; 1: s = 2 x_f - x_{f-1} + acc, f - 1 the
// tensor's previous frame (x_0 at frame 0).  ADD: rhs += diag s; otherwise rhs = diag s, the very value the sum adds
template <bool ADD>
__global__ __launch_bounds__(256) void k_gs_inertia(CpWorld w, int f0, int fj, int n_sel, long long n_verts, const double* __restrict__ diag,
                                                    int mode, double acc0, double acc1, double acc2, double* __restrict__ rhs) {
    constexpr int RUN = GS_VB * 3, ROW = RUN + 1;
    __shared__ double stage[64 * ROW];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t0 = (int)blockIdx.y * 64;
    // a lane past the last selected frame recomputes frame f0 (an address inside the tensor); its row is never written out
    const long long f = (long long)f0 + (long long)(t0 + lane < n_sel ? t0 + lane : 0) * fj;
    const long long fp = f > 0 ? f - 1 : 0;
    const double acc[3] = {acc0, acc1, acc2};
    const long long v_base = (long long)blockIdx.x * GS_VB;
    for (int j = wid; j < GS_VB; j += 4) {
        const long long v = v_base + j;
        if (v >= n_verts) break;                    // the same in every lane
        double x[3], xp[3];
        cp_pos(w, f, (int)v, x);
        const double dg = diag[v];
        if (mode == 1) {
            cp_pos(w, fp, (int)v, xp);
#pragma unroll
            for (int d = 0; d < 3; ++d) x[d] = 2.0 * x[d] - xp[d];
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) stage[lane * ROW + j * 3 + d] = dg * (x[d] + acc[d]);
    }
    __syncthreads();
    const int nv = n_verts - v_base < GS_VB ? (int)(n_verts - v_base) : GS_VB;
    const int nf = n_sel - t0 < 64 ? n_sel - t0 : 64;
    const int run = nv * 3;
    for (int e = threadIdx.x; e < 64 * RUN; e += 256) {
        const int fl = e / RUN, k = e % RUN;
        if (fl < nf && k < run) {
            double* o = rhs + ((long long)(t0 + fl) * n_verts + v_base) * 3 + k;
            if (ADD) *o += stage[fl * ROW + k];
            else *o = stage[fl * ROW + k];
        }
    }
}

void asb_gs_inertia_launch(asb_ctx* ctx, const CpWorld& w, int f0, int fj, int n_sel, long long n, const double* diag_dev, int mode,
                           const double* acc3, bool add, double* out) {
    const dim3 grid((unsigned)((n + GS_VB - 1) / GS_VB), (unsigned)((n_sel + 63) / 64));
    if (add)
        hipLaunchKernelGGL(k_gs_inertia<true>, grid, dim3(256), 0, ctx->stream, w, f0, fj, n_sel, n, diag_dev, mode, acc3[0], acc3[1], acc3[2], out);
    else
        hipLaunchKernelGGL(k_gs_inertia<false>, grid, dim3(256), 0, ctx->stream, w, f0, fj, n_sel, n, diag_dev, mode, acc3[0], acc3[1], acc3[2], out);
}

extern "C" int asb_gstep_inertia(asb_ctx* ctx, int which, int64_t f0, int64_t f1, int64_t fj, const double* inv_massL, int add_mean, double psf,
                                 const double* diag, int mode, const double* acc3, double* rhs_dev) {
    if (!ctx || !diag || !acc3 || !rhs_dev) return ASB_ERR_ARG;
    if (mode != 0 && mode != 1) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_gstep_inertia: mode %d (0: s = x, 1: s = 2 x - x_prev)", mode);
    CpWorld w;
    int64_t n_sel;
    int rc;
    if ((rc = asb_world_frames(ctx, "asb_gstep_inertia", which, f0, f1, fj, add_mean, psf, &w, &n_sel))) return rc;
    if ((n_sel + 63) / 64 > 65535) ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_gstep_inertia: %lld frames in one call (at most %d)", (long long)n_sel, 65535 * 64);
    const int64_t n = ctx->n_loc;
    for (int64_t v = 0; v < n; ++v)
        if (!std::isfinite(diag[v])) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_gstep_inertia: diag[%lld] is not finite", (long long)v);
    if (!std::isfinite(acc3[0]) || !std::isfinite(acc3[1]) || !std::isfinite(acc3[2])) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_gstep_inertia: acc is not finite");
    if ((rc = asb_cproj_invm(ctx, inv_massL, &w))) return rc;
    if ((rc = asb_alloc(ctx, &ctx->gs_diag, (size_t)n))) return rc;
    ASB_HIP(ctx, hipMemcpyAsync(ctx->gs_diag, diag, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    asb_gs_inertia_launch(ctx, w, (int)f0, (int)fj, (int)n_sel, (long long)n, ctx->gs_diag, mode, acc3, true, rhs_dev);
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));          // the host arrays may go; the caller owns rhs_dev
    return ASB_OK;
}

// test hook: the n x n block of the context's A^-1, row-major, to the host
extern "C" int asb_test_gstep_inverse(asb_ctx* ctx, double* out_host, int64_t n) {
    if (!ctx || !out_host) return ASB_ERR_ARG;
    if (asb_gslab_n(ctx) > 0) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_test_gstep_inverse: the context holds the slab factor, no explicit inverse");
    if (ctx->gs_n < 1 || n != ctx->gs_n) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_test_gstep_inverse: the inverse has %lld rows, not %lld", (long long)ctx->gs_n, (long long)n);
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    ASB_HIP(ctx, hipMemcpy2DAsync(out_host, (size_t)n * sizeof(double), ctx->gs_Ainv, (size_t)ctx->gs_Np * sizeof(double), (size_t)n * sizeof(double),
                                  (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ASB_OK;
}
