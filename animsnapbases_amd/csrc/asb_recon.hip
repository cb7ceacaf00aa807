// Reconstruction-error sweeps over prefixes of a basis (posComponents.test_convergence, snapbases/posComponents.py:192-249)
// and the least-squares projection of a held-out animation onto the position basis.
//
// k_recon_sweep reads a vertex-major tensor T (rows r = 3 v + d, ld doubles each) ONCE.  A wave owns RC_VT vertices (3 RC_VT
// rows) and 64 RC_NF frames at a time, RC_NF frames per lane; it keeps those elements of T and of the running reconstruction
// sum_{j < k} A[j][f] B[j][r] in registers and adds one rank-1 term per k (f64 FMA).  At every sweep point k_s the lane's
// squared errors per axis and its largest |error| are reduced over the wave (DPP) and added to the wave's own slot row in LDS;
// the block sums its waves in a fixed order into per-block partials, and k_recon_final reduces those over the blocks in
// block order.  No atomics: repeated calls give bit-identical results.
#include "asb_common.h"

#include <cmath>
#include <vector>

#define RC_VT 2         // vertices per wave work unit
#define RC_NF 4         // frames per lane (strided by 64: the wave's loads of a row are coalesced)
#define RC_WAVES 4      // waves per block
#define RC_MAX_S 1024   // sweep points per call (LDS: RC_WAVES x (S + 1) x 4 doubles)

// slot s < S: [sum e_x^2, sum e_y^2, sum e_z^2, max |e|]; slot S: [sum T_x^2, sum T_y^2, sum T_z^2, max T]
__global__ __launch_bounds__(256) void k_recon_sweep(const double* __restrict__ T, long long ldt, int F, long long n_loc,
                                                     const double* __restrict__ A, long long lda,
                                                     const double* __restrict__ B, long long ldb,
                                                     const int* __restrict__ ks, int S, long long n_units, int n_fchunks,
                                                     double* __restrict__ part) {
    extern __shared__ double rc_lds[];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nslot = (S + 1) * 4;
    double* my = rc_lds + (size_t)wid * nslot;
    for (int i = lane; i < nslot; i += 64) my[i] = (i == S * 4 + 3) ? -INFINITY : 0.0;
    __syncthreads();

    for (long long u = (long long)blockIdx.x * RC_WAVES + wid; u < n_units; u += (long long)gridDim.x * RC_WAVES) {
        const long long vbase = (u / n_fchunks) * RC_VT;
        const int f0 = (int)(u % n_fchunks) * 64 * RC_NF + lane;
        bool fok[RC_NF], rok[RC_VT * 3];
#pragma unroll
        for (int q = 0; q < RC_NF; ++q) fok[q] = f0 + 64 * q < F;
#pragma unroll
        for (int i = 0; i < RC_VT * 3; ++i) rok[i] = vbase + i / 3 < n_loc;
        double t[RC_VT * 3][RC_NF], a[RC_VT * 3][RC_NF];
        double n3[3] = {0.0, 0.0, 0.0}, mt = -INFINITY;
#pragma unroll
        for (int i = 0; i < RC_VT * 3; ++i)
#pragma unroll
            for (int q = 0; q < RC_NF; ++q) {
                const bool ok = rok[i] && fok[q];
                t[i][q] = ok ? T[(3 * vbase + i) * ldt + f0 + 64 * q] : 0.0;
                a[i][q] = 0.0;
                n3[i % 3] = fma(t[i][q], t[i][q], n3[i % 3]);
                if (ok) mt = fmax(mt, t[i][q]);
            }
        wave_sum_dpp<3>(n3);
        mt = wave_max_dpp(mt);
        if (lane == 0) {
            my[S * 4 + 0] += n3[0];
            my[S * 4 + 1] += n3[1];
            my[S * 4 + 2] += n3[2];
            my[S * 4 + 3] = fmax(my[S * 4 + 3], mt);
        }
        int kprev = 0;
        for (int s = 0; s < S; ++s) {
            const int kn = ks[s];
#pragma unroll 2
            for (int k = kprev; k < kn; ++k) {          // + A[k] (x) B[k] on this tile (masked entries stay exactly 0)
                double w[RC_NF], c[RC_VT * 3];
#pragma unroll
                for (int q = 0; q < RC_NF; ++q) w[q] = fok[q] ? A[(long long)k * lda + f0 + 64 * q] : 0.0;
#pragma unroll
                for (int i = 0; i < RC_VT * 3; ++i) c[i] = rok[i] ? B[(long long)k * ldb + 3 * vbase + i] : 0.0;
#pragma unroll
                for (int i = 0; i < RC_VT * 3; ++i)
#pragma unroll
                    for (int q = 0; q < RC_NF; ++q) a[i][q] = fma(w[q], c[i], a[i][q]);
            }
            kprev = kn;
            double e3[3] = {0.0, 0.0, 0.0}, m = 0.0;
#pragma unroll
            for (int i = 0; i < RC_VT * 3; ++i)
#pragma unroll
                for (int q = 0; q < RC_NF; ++q) {
                    const double d = t[i][q] - a[i][q];
                    e3[i % 3] = fma(d, d, e3[i % 3]);
                    m = fmax(m, fabs(d));
                }
            wave_sum_dpp<3>(e3);
            m = wave_max_dpp(m);
            if (lane == 0) {
                my[s * 4 + 0] += e3[0];
                my[s * 4 + 1] += e3[1];
                my[s * 4 + 2] += e3[2];
                my[s * 4 + 3] = fmax(my[s * 4 + 3], m);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nslot; i += blockDim.x) {
        const bool is_max = (i & 3) == 3;
        double v = rc_lds[i];
        for (int w = 1; w < RC_WAVES; ++w) {
            const double x = rc_lds[(size_t)w * nslot + i];
            v = is_max ? fmax(v, x) : v + x;
        }
        part[(size_t)blockIdx.x * nslot + i] = v;
    }
}

__global__ __launch_bounds__(256) void k_recon_final(const double* __restrict__ part, int nblk, int nslot, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nslot) return;
    const bool is_max = (i & 3) == 3;
    double v = part[i];
    for (int b = 1; b < nblk; ++b) {
        const double x = part[(size_t)b * nslot + i];
        v = is_max ? fmax(v, x) : v + x;
    }
    out[i] = v;
}

// held-out frames f0 .. f0 + fc of the staged (F, n_loc, 3) shard -> Y rows (3 v + d) of ld doubles, transformed like the
// training tensor: mass weighting (posSnapshots.py:82), the training mean row (:168) and pre_scale_factor (:172)
__global__ __launch_bounds__(256) void k_heldout_prep(const double* __restrict__ stage, long long F, long long n_loc,
                                                      const double* __restrict__ massL, const double* __restrict__ mean,
                                                      int subtract, double scale, double* __restrict__ Y, long long ld) {
    const long long rows = 3 * n_loc, total = rows * F;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const long long r = e / F, f = e % F;
        double x = stage[f * rows + r];
        if (massL) x *= massL[r / 3];
        if (subtract) x -= mean[r];
        Y[r * ld + f] = x * scale;
    }
}

// Q = T C (K x n3): rows of the prefix-orthonormal basis; T lower triangular, dependent rows zero
__global__ __launch_bounds__(256) void k_ho_rows(const double* __restrict__ Tm, int K, const double* __restrict__ C, long long n3,
                                                 double* __restrict__ Q) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n3) return;
    for (int k0 = 0; k0 < K; k0 += 16) {
        double acc[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 0.0;
        const int kend = k0 + 16 < K ? k0 + 16 : K;
        for (int i = 0; i < kend; ++i) {
            const double c = C[(long long)i * n3 + r];
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (k0 + j < kend && i <= k0 + j) acc[j] = fma(Tm[(k0 + j) * K + i], c, acc[j]);
        }
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (k0 + j < kend) Q[(long long)(k0 + j) * n3 + r] = acc[j];
    }
}

// Zt[k][f] = sum_{i <= k} T[k][i] P[f][i]  (Z = P T^T, stored K x ld like the weights of the deflation)
__global__ __launch_bounds__(256) void k_ho_coef(const double* __restrict__ Tm, int K, const double* __restrict__ P, long long F,
                                                 double* __restrict__ Zt, long long ld) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= F * K) return;
    const int k = (int)(e / F);
    const long long f = e % F;
    double acc = 0.0;
    for (int i = 0; i <= k; ++i) acc = fma(Tm[k * K + i], P[f * K + i], acc);
    Zt[(long long)k * ld + f] = acc;
}

// least-squares weights on the original components: W = Z T (F x K), W[f][k] = sum_{j >= k} Zt[j][f] T[j][k]
__global__ __launch_bounds__(256) void k_ho_weights(const double* __restrict__ Tm, int K, const double* __restrict__ Zt, long long ld,
                                                    long long F, double* __restrict__ W) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= F * K) return;
    const long long f = e / K;
    const int k = (int)(e % K);
    double acc = 0.0;
    for (int j = k; j < K; ++j) acc = fma(Zt[(long long)j * ld + f], Tm[j * K + k], acc);
    W[e] = acc;
}

static int grid_for(long long n) { return (int)((n + 255) / 256 < 65535 ? (n + 255) / 256 : 65535); }

extern "C" int asb_heldout_upload(asb_ctx* ctx, const double* Y, int64_t F, int64_t N_glob, int64_t v0, int64_t n_loc,
                                  const double* massL, int subtract, double pre_scale_factor) {
    if (!ctx || !Y || F < 1 || !ctx->X) return ASB_ERR_ARG;
    if (n_loc != ctx->n_loc || v0 != ctx->v0 || N_glob != ctx->N_glob)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_heldout_upload: shard [%lld, +%lld) of %lld vertices, the training tensor has [%lld, +%lld) of %lld",
                 (long long)v0, (long long)n_loc, (long long)N_glob, (long long)ctx->v0, (long long)ctx->n_loc, (long long)ctx->N_glob);
    if (subtract && !ctx->have_mean) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_heldout_upload: no training mean on the device");
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    const long long Fp = (F + 15) / 16 * 16, rows = 3 * n_loc;
    int rc;
    if ((rc = asb_alloc(ctx, &ctx->ho_Y, (size_t)rows * Fp))) return rc;
    ctx->ho_F = F;
    ctx->ho_Fp = Fp;
    ctx->ho_K = 0;
    ASB_HIP(ctx, hipMemsetAsync(ctx->ho_Y, 0, (size_t)rows * Fp * sizeof(double), ctx->stream));
    asb_tmp<double> stage, mdev;
    if ((rc = asb_stage_shard(ctx, Y, F, N_glob, v0, n_loc, massL, stage, mdev))) return rc;
    hipLaunchKernelGGL(k_heldout_prep, dim3(grid_for(rows * F)), dim3(256), 0, ctx->stream, stage.get(), (long long)F, (long long)n_loc,
                       mdev.get(), ctx->mean, subtract, pre_scale_factor, ctx->ho_Y, Fp);
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ASB_OK;
}

extern "C" int asb_heldout_gram(asb_ctx* ctx, double* P_dev, double* G_dev) {
    if (!ctx || !ctx->ho_Y || !ctx->comps || ctx->K < 1) return ASB_ERR_ARG;
    const int64_t K = ctx->K, n3 = 3 * ctx->n_loc, F = ctx->ho_F;
    int rc;
    if ((rc = asb_alloc(ctx, &ctx->ho_Ct, (size_t)n3 * K))) return rc;
    if ((rc = asb_alloc(ctx, &ctx->ho_P, (size_t)F * K))) return rc;
    if ((rc = asb_alloc(ctx, &ctx->ho_G, (size_t)K * K))) return rc;
    double* Pout = P_dev ? P_dev : ctx->ho_P;
    double* Gout = G_dev ? G_dev : ctx->ho_G;
    ctx->ho_K = 0;
    // the same MFMA products as asb_splocs_gram: P = Y^T C^T (F x K), G = C C^T (K x K)
    if ((rc = asb_transpose(ctx, ctx->comps, K, n3, ctx->ho_Ct))) return rc;
    if (K >= 32 && !(K & 1)) rc = asb_gemm_tn_big(ctx, ctx->ho_Y, ctx->ho_Fp, ctx->ho_Ct, K, n3, (int)F, (int)K, Pout);
    else rc = asb_gemm_tn(ctx, ctx->ho_Y, ctx->ho_Fp, ctx->ho_Ct, K, n3, (int)F, (int)K, Pout);
    if (rc) return rc;
    return asb_gemm_tn(ctx, ctx->ho_Ct, K, ctx->ho_Ct, K, n3, (int)K, (int)K, Gout);
}

// G = L L^T with dependent components dropped: T = L^-1 row by row, a row whose pivot is at or below tol stays zero
static int64_t chol_tinv_drop(const std::vector<double>& G, int64_t K, double tol, std::vector<double>& T) {
    std::vector<double> L((size_t)K * K, 0.0);
    T.assign((size_t)K * K, 0.0);
    int64_t dropped = 0;
    for (int64_t k = 0; k < K; ++k) {
        for (int64_t j = 0; j < k; ++j) {
            if (L[j * K + j] == 0.0) continue;
            double s = G[k * K + j];
            for (int64_t i = 0; i < j; ++i) s -= L[k * K + i] * L[j * K + i];
            L[k * K + j] = s / L[j * K + j];
        }
        double d = G[k * K + k];
        for (int64_t i = 0; i < k; ++i) d -= L[k * K + i] * L[k * K + i];
        if (!(d > tol)) {           // (also NaN)
            for (int64_t i = 0; i < k; ++i) L[k * K + i] = 0.0;
            ++dropped;
            continue;
        }
        const double lkk = std::sqrt(d);
        L[k * K + k] = lkk;
        for (int64_t i = 0; i <= k; ++i) {
            double s = (i == k) ? 1.0 : 0.0;
            for (int64_t j = i; j < k; ++j) s -= L[k * K + j] * T[j * K + i];
            T[k * K + i] = s / lkk;
        }
    }
    return dropped;
}

extern "C" int asb_heldout_factor(asb_ctx* ctx, const double* P_dev, const double* G_dev, int64_t* n_dropped) {
    if (!ctx || !ctx->ho_Y || !ctx->comps || ctx->K < 1 || !ctx->ho_P) return ASB_ERR_ARG;
    const int64_t K = ctx->K, n3 = 3 * ctx->n_loc, F = ctx->ho_F;
    const double* P = P_dev ? P_dev : ctx->ho_P;
    const double* Gd = G_dev ? G_dev : ctx->ho_G;
    std::vector<double> G((size_t)K * K), T;
    ASB_HIP(ctx, hipMemcpyAsync(G.data(), Gd, G.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    double tr = 0.0;
    for (int64_t k = 0; k < K; ++k) tr += G[k * K + k];
    const double tol = 3.0 * (double)ctx->N_glob * 2.220446049250313e-16 * tr;
    const int64_t dropped = chol_tinv_drop(G, K, tol, T);
    int rc;
    if ((rc = asb_alloc(ctx, &ctx->ho_T, (size_t)K * K))) return rc;
    if ((rc = asb_alloc(ctx, &ctx->ho_Q, (size_t)K * n3))) return rc;
    if ((rc = asb_alloc(ctx, &ctx->ho_Zt, (size_t)K * ctx->ho_Fp))) return rc;
    ASB_HIP(ctx, hipMemcpyAsync(ctx->ho_T, T.data(), T.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemsetAsync(ctx->ho_Zt, 0, (size_t)K * ctx->ho_Fp * sizeof(double), ctx->stream));
    hipLaunchKernelGGL(k_ho_rows, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, ctx->stream, ctx->ho_T, (int)K, ctx->comps,
                       (long long)n3, ctx->ho_Q);
    hipLaunchKernelGGL(k_ho_coef, dim3((unsigned)((F * K + 255) / 256)), dim3(256), 0, ctx->stream, ctx->ho_T, (int)K, P, (long long)F,
                       ctx->ho_Zt, (long long)ctx->ho_Fp);
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));      // (T lives in a host vector)
    ctx->ho_K = K;
    if (n_dropped) *n_dropped = dropped;
    return ASB_OK;
}

extern "C" int asb_heldout_weights(asb_ctx* ctx, double* W_out) {
    if (!ctx || !W_out || ctx->ho_K < 1 || ctx->ho_K != ctx->K) return ASB_ERR_ARG;
    const int64_t K = ctx->ho_K, F = ctx->ho_F;
    int rc;
    if ((rc = asb_alloc(ctx, &ctx->ho_W, (size_t)F * K))) return rc;
    hipLaunchKernelGGL(k_ho_weights, dim3((unsigned)((F * K + 255) / 256)), dim3(256), 0, ctx->stream, ctx->ho_T, (int)K, ctx->ho_Zt,
                       (long long)ctx->ho_Fp, (long long)F, ctx->ho_W);
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipMemcpyAsync(W_out, ctx->ho_W, (size_t)F * K * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ASB_OK;
}

int asb_recon_operands(asb_ctx* ctx, const char* who, const char* idx, int which, int64_t kmax, RcOperands* o) {
    if (which == 0) {
        // the greedy weights of the deflation (K_W rows of Fp) and the device-resident basis
        const int64_t kw = (int64_t)(asb_capacity(ctx, &ctx->W) / ctx->Fp);
        if (kmax > ctx->K || kmax > kw)
            ASB_FAIL(ctx, ASB_ERR_ARG, "%s: %s = %lld but %lld components and %lld weight columns", who, idx, (long long)kmax,
                     (long long)ctx->K, (long long)kw);
        *o = {ctx->X, ctx->W, ctx->comps, ctx->Fp, ctx->Fp, (int)ctx->F};
    } else if (which == 1) {
        if (!ctx->ho_Y || ctx->ho_K != ctx->K) ASB_FAIL(ctx, ASB_ERR_ARG, "%s: no factorised held-out animation for this basis", who);
        if (kmax > ctx->K) ASB_FAIL(ctx, ASB_ERR_ARG, "%s: %s = %lld but %lld components", who, idx, (long long)kmax, (long long)ctx->K);
        *o = {ctx->ho_Y, ctx->ho_Zt, ctx->ho_Q, ctx->ho_Fp, ctx->ho_Fp, (int)ctx->ho_F};
    } else {
        return ASB_ERR_ARG;
    }
    return ASB_OK;
}

extern "C" int asb_recon_sweep(asb_ctx* ctx, int which, const int64_t* ks, int64_t S, double* sums_out, double* max_out,
                               double* norms_out) {
    if (!ctx || !ks || S < 1 || !ctx->X || !ctx->comps) return ASB_ERR_ARG;
    if (S > RC_MAX_S) ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_recon_sweep: %lld sweep points (at most %d per call)", (long long)S, RC_MAX_S);
    for (int64_t s = 0; s < S; ++s)
        if (ks[s] < 0 || (s && ks[s] <= ks[s - 1])) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_recon_sweep: sweep points must increase from 0");
    const int64_t kmax = ks[S - 1];
    RcOperands o;
    int rc;
    if ((rc = asb_recon_operands(ctx, "asb_recon_sweep", "k", which, kmax, &o))) return rc;
    const int nslot = (int)(S + 1) * 4;
    const int n_fchunks = (o.F + 64 * RC_NF - 1) / (64 * RC_NF);
    const long long n_units = (ctx->n_loc + RC_VT - 1) / RC_VT * n_fchunks;
    long long nblk = (n_units + RC_WAVES - 1) / RC_WAVES;
    if (nblk > 4LL * ctx->n_cu) nblk = 4LL * ctx->n_cu;
    if ((rc = asb_alloc(ctx, &ctx->rc_part, (size_t)(nblk + 1) * nslot))) return rc;
    if ((rc = asb_alloc(ctx, &ctx->rc_ks, (size_t)S))) return rc;
    std::vector<int> k32(ks, ks + S);
    std::vector<double> h((size_t)nslot);
    ASB_HIP(ctx, hipMemcpyAsync(ctx->rc_ks, k32.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    const size_t lds = (size_t)RC_WAVES * nslot * sizeof(double);
    if (lds > 48 * 1024) ASB_HIP(ctx, hipFuncSetAttribute((const void*)k_recon_sweep, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    double* out = ctx->rc_part + (size_t)nblk * nslot;
    hipLaunchKernelGGL(k_recon_sweep, dim3((unsigned)nblk), dim3(64 * RC_WAVES), lds, ctx->stream, o.T, o.ldt, o.F, (long long)ctx->n_loc,
                       o.A, o.lda, o.B, (long long)(3 * ctx->n_loc), ctx->rc_ks, (int)S, n_units, n_fchunks, ctx->rc_part);
    hipLaunchKernelGGL(k_recon_final, dim3((unsigned)((nslot + 255) / 256)), dim3(256), 0, ctx->stream, ctx->rc_part, (int)nblk, nslot,
                       out);
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipMemcpyAsync(h.data(), out, (size_t)nslot * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t s = 0; s < S; ++s) {
        if (sums_out)
            for (int d = 0; d < 3; ++d) sums_out[s * 3 + d] = h[s * 4 + d];
        if (max_out) max_out[s] = h[s * 4 + 3];
    }
    if (norms_out)
        for (int d = 0; d < 4; ++d) norms_out[d] = h[S * 4 + d];
    return ASB_OK;
}
