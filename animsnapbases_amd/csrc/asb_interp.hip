// Interpolation-error sweeps for constraint bases (generate_figures/nl_reduction_tests.py:117-225, run_geom_tests, with
// constraintsComponents.geom_constructed, snapbases/constraintsComponents.py:489-521, and the metrics of :524-556).
//
// For sweep points s = 0 .. S-1 (r p = rp_s basis vectors, |Pt_s| = npt_s interpolation rows) and each coordinate l:
//   C_{s,l} = M_{s,l} B_l[:npt_s]             (rp_s x F; M = (A^T A)^-1 A^T from the host's LU, B = the rows of T at Pt)
//   E_{s,l} = T_l - V_l[:, :rp_s] C_{s,l}     (n_loc x F; never written)
// and per s the per-axis sums of E^2 and max |E|, plus once per call sum T_d^2 per axis and the signed max T.
//
// k_interp_coef forms every C of a chunk (one block per row of C and 256 frames).  k_interp_sweep is a persistent f64 MFMA
// GEMM with a fused epilogue: a block owns a 64-element x 128-frame tile of one coordinate at a time, loads the tile of T into
// registers ONCE (in the v_mfma_f64_16x16x4_f64 C/D layout) and runs every sweep point of the chunk over it: V_l and C_s stream
// through double-buffered LDS stages of 16 basis vectors (the k_syrk_tn pattern), each wave a 32 x 64 sub-tile = 2 x 4
// accumulators.  After a sweep point the waves reduce (T - acc)^2 and |T - acc| with DPP and add them to their own LDS slot
// row; the block sums its waves in order into per-block partials and k_interp_final sums the blocks in block order.  No
// atomics: repeated calls are bit-identical.
#include "asb_common.h"

#include <cmath>
#include <vector>

typedef double d4 __attribute__((ext_vector_type(4)));

#define IS_BE 64        // elements per block tile
#define IS_BF 128       // frames per block tile
#define IS_KC 16        // basis vectors per LDS stage
#define IS_LDV 80       // LDS row strides (doubles): the four k-rows a wave reads per instruction alternate bank halves
#define IS_LDC 144
#define IS_MAX_S 64     // sweep points per call

// slot s < S: [sum e_x^2, sum e_y^2, sum e_z^2, max |e|]; slot S: [sum T_x^2, sum T_y^2, sum T_z^2, max T]
__global__ __launch_bounds__(256, 2) void k_interp_sweep(const double* __restrict__ T, long long ldt, int F, long long n_loc,
                                                         const double* __restrict__ V, long long ldv,
                                                         const double* __restrict__ C, const long long* __restrict__ coff,
                                                         const int* __restrict__ rps, int S, int n_ft, long long n_tiles,
                                                         double* __restrict__ part) {
    __shared__ double Vs[2][IS_KC][IS_LDV];
    __shared__ double Cs[2][IS_KC][IS_LDC];
    extern __shared__ double is_slots[];
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int nslot = (S + 1) * 4;
    double* my = is_slots + (size_t)wave * nslot;
    for (int i = lane; i < nslot; i += 64) my[i] = (i == S * 4 + 3) ? -INFINITY : 0.0;
    __syncthreads();

    for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int l = (int)(t % 3);
        const long long et = t / 3 / n_ft;
        const int ft = (int)(t / 3 % n_ft);
        const long long e0 = et * IS_BE;
        const int f0 = ft * IS_BF;
        // T tile in the accumulator layout: row e0 + 32 wr + 16 x + g + 4 q, frame f0 + 64 wc + 16 y + li
        double tv[2][4][4];
        double n2 = 0.0, mt = -INFINITY;
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const long long e = e0 + 32 * wr + 16 * x + g + 4 * q;
                    const int f = f0 + 64 * wc + 16 * y + li;
                    const bool ok = e < n_loc && f < F;
                    const double v = ok ? T[(3 * e + l) * ldt + f] : 0.0;
                    tv[x][y][q] = v;
                    n2 = fma(v, v, n2);
                    if (ok) mt = fmax(mt, v);
                }
        {
            double a1[1] = {n2};
            wave_sum_dpp<1>(a1);
            mt = wave_max_dpp(mt);
            if (lane == 0) {
                my[S * 4 + l] += a1[0];
                my[S * 4 + 3] = fmax(my[S * 4 + 3], mt);
            }
        }
        // this thread's share of a stage: V rows jr + 4 q (element tid & 63), C rows jc + 2 q (frame tid & 127)
        const long long ev = e0 + (tid & 63);
        const int jr = tid >> 6;
        const int fc = f0 + (tid & 127), jc = tid >> 7;
        const bool evok = ev < n_loc, fcok = fc < F;
        const double* pv = V + 3 * ev + l;
        for (int s = 0; s < S; ++s) {
            const int rp = rps[s];
            const double* pc = C + coff[s] + (long long)l * rp * F + fc;
            double rv[4], rc[8];
            auto fetch = [&](int j0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int j = j0 + jr + 4 * q;
                    rv[q] = (evok && j < rp) ? pv[(long long)j * ldv] : 0.0;
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int j = j0 + jc + 2 * q;
                    rc[q] = (fcok && j < rp) ? pc[(long long)j * F] : 0.0;
                }
            };
            auto stash = [&](int buf) {
#pragma unroll
                for (int q = 0; q < 4; ++q) Vs[buf][jr + 4 * q][tid & 63] = rv[q];
#pragma unroll
                for (int q = 0; q < 8; ++q) Cs[buf][jc + 2 * q][tid & 127] = rc[q];
            };
            d4 acc[2][4];
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) acc[x][y] = d4{0.0, 0.0, 0.0, 0.0};
            fetch(0);
            stash(0);
            __syncthreads();
            int cur = 0;
            for (int j0 = 0; j0 < rp; j0 += IS_KC) {
                const bool more = j0 + IS_KC < rp;
                if (more) fetch(j0 + IS_KC);
#pragma unroll
                for (int ks = 0; ks < IS_KC / 4; ++ks) {
                    double a[2], b[4];
#pragma unroll
                    for (int x = 0; x < 2; ++x) a[x] = Vs[cur][ks * 4 + g][32 * wr + 16 * x + li];
#pragma unroll
                    for (int y = 0; y < 4; ++y) b[y] = Cs[cur][ks * 4 + g][64 * wc + 16 * y + li];
#pragma unroll
                    for (int x = 0; x < 2; ++x)
#pragma unroll
                        for (int y = 0; y < 4; ++y) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[x], b[y], acc[x][y], 0, 0, 0);
                }
                if (more) stash(cur ^ 1);
                __syncthreads();
                cur ^= 1;
            }
            // masked rows / frames: T and the product are both exactly 0 there
            double e2[1] = {0.0}, m = 0.0;
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const double d = tv[x][y][q] - acc[x][y][q];
                        e2[0] = fma(d, d, e2[0]);
                        m = fmax(m, fabs(d));
                    }
            wave_sum_dpp<1>(e2);
            m = wave_max_dpp(m);
            if (lane == 0) {
                my[s * 4 + l] += e2[0];
                my[s * 4 + 3] = fmax(my[s * 4 + 3], m);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < nslot; i += blockDim.x) {
        const bool is_max = (i & 3) == 3;
        double v = is_slots[i];
        for (int w = 1; w < 4; ++w) {
            const double x = is_slots[(size_t)w * nslot + i];
            v = is_max ? fmax(v, x) : v + x;
        }
        part[(size_t)blockIdx.x * nslot + i] = v;
    }
}

__global__ __launch_bounds__(256) void k_interp_final(const double* __restrict__ part, int nblk, int nslot, double* __restrict__ out) {
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

// C row r (sweep point s, coordinate l, basis vector j), frames f: sum_i M[moff_r + i] B[i][f][l], i < npt_r (in order)
__global__ __launch_bounds__(256) void k_interp_coef(const double* __restrict__ M, const double* __restrict__ B, int F,
                                                     const long long* __restrict__ rmoff, const int* __restrict__ rnpt,
                                                     const long long* __restrict__ rcoff, const int* __restrict__ rl, int nfb,
                                                     double* __restrict__ C) {
    const long long row = blockIdx.x / nfb;
    const int f = (int)(blockIdx.x % nfb) * 256 + threadIdx.x;
    if (f >= F) return;
    const double* pm = M + rmoff[row];
    const int n = rnpt[row], l = rl[row];
    const double* pb = B + 3LL * f + l;
    double acc = 0.0;
    for (int i = 0; i < n; ++i) acc = fma(pm[i], pb[3LL * F * i], acc);
    C[rcoff[row] + f] = acc;
}

// out[i][f][l] = T[3 (gidx[i] - v0) + l][f] of this shard; rows another rank owns are 0
__global__ __launch_bounds__(256) void k_rows_gather(const double* __restrict__ T, long long ldt, int F, long long v0, long long n_loc,
                                                     const long long* __restrict__ gidx, long long n, double* __restrict__ out) {
    const long long total = n * F * 3;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const long long i = e / (3LL * F);
        const int f = (int)(e / 3 % F), l = (int)(e % 3);
        const long long r = gidx[i] - v0;
        out[e] = (r >= 0 && r < n_loc) ? T[(3 * r + l) * ldt + f] : 0.0;
    }
}

// the tensor of `which`: 0 the prepared snapshots X, 1 the held-out frames of asb_heldout_upload
static int interp_tensor(asb_ctx* ctx, int which, const double** T, long long* ldt, int* F) {
    if (which == 0 && ctx->X) {
        *T = ctx->X, *ldt = ctx->Fp, *F = (int)ctx->F;
        return ASB_OK;
    }
    if (which == 1 && ctx->ho_Y) {
        *T = ctx->ho_Y, *ldt = ctx->ho_Fp, *F = (int)ctx->ho_F;
        return ASB_OK;
    }
    ASB_FAIL(ctx, ASB_ERR_ARG, "interpolation sweep: no %s tensor on the device", which == 0 ? "snapshot" : "held-out");
}

extern "C" int asb_rows_gather(asb_ctx* ctx, int which, const int64_t* gidx, int64_t n, double* out, int* owned_out) {
    if (!ctx || !gidx || n < 1 || !out) return ASB_ERR_ARG;
    const double* T;
    long long ldt;
    int F, rc;
    if ((rc = interp_tensor(ctx, which, &T, &ldt, &F))) return rc;
    for (int64_t i = 0; i < n; ++i) {
        if (gidx[i] < 0 || gidx[i] >= ctx->N_glob)
            ASB_FAIL(ctx, ASB_ERR_ARG, "asb_rows_gather: row %lld of %lld", (long long)gidx[i], (long long)ctx->N_glob);
        if (owned_out) owned_out[i] = gidx[i] >= ctx->v0 && gidx[i] < ctx->v0 + ctx->n_loc;
    }
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    if ((rc = asb_alloc(ctx, &ctx->is_idx, (size_t)n))) return rc;
    if ((rc = asb_alloc(ctx, &ctx->is_B, (size_t)n * F * 3))) return rc;
    ASB_HIP(ctx, hipMemcpyAsync(ctx->is_idx, gidx, (size_t)n * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    const long long total = (long long)n * F * 3;
    const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_rows_gather, dim3(grid), dim3(256), 0, ctx->stream, T, ldt, F, (long long)ctx->v0, (long long)ctx->n_loc,
                       ctx->is_idx, (long long)n, ctx->is_B);
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipMemcpyAsync(out, ctx->is_B, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ASB_OK;
}

extern "C" int asb_interp_sweep(asb_ctx* ctx, int which, const int64_t* rp, const int64_t* npt, int64_t S, const double* M,
                                const double* B, int64_t nb, double* sums_out, double* max_out, double* norms_out) {
    if (!ctx || !rp || !npt || S < 1 || !M || !B || nb < 1 || !ctx->comps) return ASB_ERR_ARG;
    if (S > IS_MAX_S) ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_interp_sweep: %lld sweep points (at most %d per call)", (long long)S, IS_MAX_S);
    const double* T;
    long long ldt;
    int F, rc;
    if ((rc = interp_tensor(ctx, which, &T, &ldt, &F))) return rc;
    // per sweep point: offsets of M_s (3 x rp x npt) and C_s (3 x rp x F); per row of C: its M row, length, C row, coordinate
    std::vector<long long> moff(S), coff(S), rmoff, rcoff;
    std::vector<int> rps(S), rnpt, rl;
    long long mtot = 0, ctot = 0;
    for (int64_t s = 0; s < S; ++s) {
        if (rp[s] < 1 || rp[s] > ctx->K || npt[s] < rp[s] || npt[s] > nb)
            ASB_FAIL(ctx, ASB_ERR_ARG, "asb_interp_sweep: sweep point %lld: %lld basis vectors (of %lld) and %lld interpolation rows (of %lld)",
                     (long long)s, (long long)rp[s], (long long)ctx->K, (long long)npt[s], (long long)nb);
        moff[s] = mtot, coff[s] = ctot, rps[s] = (int)rp[s];
        for (int l = 0; l < 3; ++l)
            for (int64_t j = 0; j < rp[s]; ++j) {
                rmoff.push_back(mtot + (l * rp[s] + j) * npt[s]);
                rcoff.push_back(ctot + (l * rp[s] + j) * (long long)F);
                rnpt.push_back((int)npt[s]);
                rl.push_back(l);
            }
        mtot += 3 * rp[s] * npt[s];
        ctot += 3 * rp[s] * (long long)F;
    }
    const long long nrows = (long long)rmoff.size();
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    if ((rc = asb_alloc(ctx, &ctx->is_M, (size_t)mtot))) return rc;
    if ((rc = asb_alloc(ctx, &ctx->is_B, (size_t)nb * F * 3))) return rc;
    if ((rc = asb_alloc(ctx, &ctx->is_C, (size_t)ctot))) return rc;
    if ((rc = asb_alloc(ctx, &ctx->is_off, (size_t)(S + 2 * nrows)))) return rc;
    if ((rc = asb_alloc(ctx, &ctx->is_int, (size_t)(S + 2 * nrows)))) return rc;
    ASB_HIP(ctx, hipMemcpyAsync(ctx->is_M, M, (size_t)mtot * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemcpyAsync(ctx->is_B, B, (size_t)nb * F * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemcpyAsync(ctx->is_off, coff.data(), S * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemcpyAsync(ctx->is_off + S, rmoff.data(), nrows * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemcpyAsync(ctx->is_off + S + nrows, rcoff.data(), nrows * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemcpyAsync(ctx->is_int, rps.data(), S * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemcpyAsync(ctx->is_int + S, rnpt.data(), nrows * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemcpyAsync(ctx->is_int + S + nrows, rl.data(), nrows * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    const int nfb = (F + 255) / 256;
    hipLaunchKernelGGL(k_interp_coef, dim3((unsigned)(nrows * nfb)), dim3(256), 0, ctx->stream, ctx->is_M, ctx->is_B, F,
                       ctx->is_off + S, ctx->is_int + S, ctx->is_off + S + nrows, ctx->is_int + S + nrows, nfb, ctx->is_C);
    ASB_CHECK_LAUNCH(ctx);

    const int nslot = (int)(S + 1) * 4;
    const int n_ft = (F + IS_BF - 1) / IS_BF;
    const long long n_tiles = (ctx->n_loc + IS_BE - 1) / IS_BE * n_ft * 3;
    long long nblk = n_tiles < 2LL * ctx->n_cu ? n_tiles : 2LL * ctx->n_cu;
    if ((rc = asb_alloc(ctx, &ctx->is_part, (size_t)(nblk + 1) * nslot))) return rc;
    const size_t lds = (size_t)4 * nslot * sizeof(double);
    ASB_HIP(ctx, hipFuncSetAttribute((const void*)k_interp_sweep, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_interp_sweep, dim3((unsigned)nblk), dim3(256), lds, ctx->stream, T, ldt, F, (long long)ctx->n_loc, ctx->comps,
                       (long long)(3 * ctx->n_loc), ctx->is_C, ctx->is_off, ctx->is_int, (int)S, n_ft, n_tiles, ctx->is_part);
    double* out = ctx->is_part + (size_t)nblk * nslot;
    hipLaunchKernelGGL(k_interp_final, dim3((unsigned)((nslot + 255) / 256)), dim3(256), 0, ctx->stream, ctx->is_part, (int)nblk, nslot,
                       out);
    ASB_CHECK_LAUNCH(ctx);
    std::vector<double> h((size_t)nslot);
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
