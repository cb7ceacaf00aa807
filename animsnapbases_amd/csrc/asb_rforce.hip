// DEIM-reduced constraint forces of the resident position animation and their error against the full term.
//
// The reference's reduced simulator replaces b = S^T p by b~_d = (S^T V_d) H_d P^T p_d per coordinate d, with
// H_d = (A^T A + la_d I)^-1 A^T, A = P^T V_d (projective_dynamics/Simulators.py:157-220 prepare_reduced_group, :222-255
// prepare_reduced_verts_bending, :366-399 get_group_reduced_term), and evaluates get_pi at the interpolation elements only.
// Here, for the frames range(f0, f1, fj) of the resident tensor:
//
//   asb_rforce_operator   once per basis: M_d = S^T V_d, three N x mp matrices, by k_st_dense -- one thread per (vertex, basis
//                         vector) walks the vertex's row of S^T in ascending column order (FMA, no atomics).  Stored transposed,
//                         (3, mpp, Np) with vertices contiguous and zero padding (mpp = mp rounded up to 4, Np = N to 32): the
//                         B operand of k_rforce_gemm, whose loads then need no bounds.  The dense N x ep matrix is never formed.
//   asb_rforce_solver     once per (m, points): H (3, r, |Pt|), r <= mp (a prefix of the operator's columns), and the rows of the
//                         SAMPLED elements' stacked projections that P^T keeps.
//   asb_rforce_run        per chunk of cw selected frames, in stream order:
//     k_cproj_em    (asb_cproj.hip) the projections of the sampled elements -- asb_cproj_setup holds only those -- element-major
//     k_rforce_coef coef_d[j][f] = sum_t H_d[j][t] p[pt_t][f][d], one thread per entry, t ascending; rows r .. rpp and the
//                   frames past the chunk's end are written as 0
//     k_rforce_gemm out[f, n, d] (+)= sum_j coef_d[j][f] M_d[n][j]: v_mfma_f64_16x16x4_f64 with A = coef^T (frames x j) and
//                   B = M^T (j x vertices), so that an accumulator row is a frame and its 16 lanes run along the vertices.  A
//                   block of 4 waves owns 64 frames x 32 vertices x 3 coordinates, stages them in LDS (odd row length) and
//                   writes per frame its contiguous run of 96 doubles.  The contraction is never split: entry (f, n, d) is one
//                   accumulator summed over j = 0 .. rpp in order, whatever tile it falls in.
// The cost of a call depends on |Pt|, mp, N and F' only.  Deterministic: repeats, accumulate onto zeros and frame sub-ranges
// give the bits of the matching slices of a full run.
//
//   asb_force_diff        the reference's three metrics of (a, b) = (full, reduced), both (F', N, 3) on the device: one block per
//                         frame reduces in a fixed tree, one block reduces the frames' records in a fixed tree.  No atomics.
#include "asb_common.h"

typedef double d4 __attribute__((ext_vector_type(4)));

#define RF_TF 64                                // frames per block of k_rforce_gemm (16 per wave)
#define RF_TN 32                                // vertices per block
#define RF_SCRATCH_BYTES (256ull << 20)         // bound on the per-chunk scratch (projections + coefficients)

// grid (blocks over N * mp), V (rows, mp, 3) -> Mt (3, mpp, Np)
__global__ __launch_bounds__(256) void k_st_dense(const int* __restrict__ ptr, const int* __restrict__ ci, const double* __restrict__ val,
                                                  const double* __restrict__ V, long long n_verts, int mp, int mpp, long long Np,
                                                  double* __restrict__ Mt) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_verts * mp) return;
    const long long v = e / mp;
    const int j = (int)(e % mp);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    const int t1 = ptr[v + 1];
    for (int t = ptr[v]; t < t1; ++t) {         // ascending columns
        const double s = val[t];
        const double* row = V + ((long long)ci[t] * mp + j) * 3;
        a0 = fma(s, row[0], a0);
        a1 = fma(s, row[1], a1);
        a2 = fma(s, row[2], a2);
    }
    Mt[(0LL * mpp + j) * Np + v] = a0;
    Mt[(1LL * mpp + j) * Np + v] = a1;
    Mt[(2LL * mpp + j) * Np + v] = a2;
}

// grid (cw / 64, rpp, 3), one wave; S: the element-major projections (row 3 local_row + d, cw doubles)
__global__ __launch_bounds__(64) void k_rforce_coef(const double* __restrict__ H, const int* __restrict__ pt, int r, int npt, int rpp,
                                                    const double* __restrict__ S, int cw, int cn, double* __restrict__ coef) {
    const int col = (int)blockIdx.x * 64 + threadIdx.x;
    const int j = blockIdx.y, d = blockIdx.z;
    double a = 0.0;
    if (j < r && col < cn) {
        const double* h = H + ((long long)d * r + j) * npt;
        for (int t = 0; t < npt; ++t) a = fma(h[t], S[(3LL * pt[t] + d) * cw + col], a);
    }
    coef[((long long)d * rpp + j) * cw + col] = a;
}

// grid (Np / RF_TN, frame tiles of the chunk); out (n_sel, n_verts, 3), rows c0 .. c0 + cn of it.  Mt rows have Np doubles
// (a multiple of RF_TN), coef rows cw doubles (a multiple of RF_TF), both with rpp rows per coordinate (a multiple of 4)
__global__ __launch_bounds__(256) void k_rforce_gemm(const double* __restrict__ Mt, long long Np, int mpp, const double* __restrict__ coef,
                                                     int cw, int rpp, int c0, int cn, long long n_verts, int accumulate,
                                                     double* __restrict__ out) {
    constexpr int RUN = RF_TN * 3, ROW = RUN + 1;
    __shared__ double stage[RF_TF * ROW];
    const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long n0 = (long long)blockIdx.x * RF_TN;
    const int t0 = (int)blockIdx.y * RF_TF;
    d4 acc[3][2];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[d][y] = d4{0.0, 0.0, 0.0, 0.0};
    const double* pa = coef + t0 + wave * 16 + i;
    const double* pb = Mt + n0 + i;
    for (int k0 = 0; k0 < rpp; k0 += 4) {
        const int k = k0 + g;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double a = pa[((long long)d * rpp + k) * cw];
            const double* b = pb + ((long long)d * mpp + k) * Np;
            acc[d][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[0], acc[d][0], 0, 0, 0);
            acc[d][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[16], acc[d][1], 0, 0, 0);
        }
    }
    // accumulator q of lane (i, g): frame g + 4 q of the wave's 16, vertex i of the 16
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int q = 0; q < 4; ++q) stage[(wave * 16 + g + 4 * q) * ROW + (16 * y + i) * 3 + d] = acc[d][y][q];
    __syncthreads();
    const int nv = n_verts - n0 < RF_TN ? (int)(n_verts - n0) : RF_TN;
    const int nf = cn - t0 < RF_TF ? cn - t0 : RF_TF;
    const int run = nv * 3;
    for (int e = threadIdx.x; e < RF_TF * RUN; e += 256) {
        const int fl = e / RUN, k = e % RUN;
        if (fl < nf && k < run) {
            double* o = out + ((long long)(c0 + t0 + fl) * n_verts + n0) * 3 + k;
            *o = accumulate ? *o + stage[fl * ROW + k] : stage[fl * ROW + k];
        }
    }
}

void asb_st_dense_launch(asb_ctx* ctx, const int* ptr, const int* ci, const double* val, const double* V, long long n_rows, int mp, int mpp,
                         long long Np, double* Mt) {
    hipLaunchKernelGGL(k_st_dense, dim3((unsigned)((n_rows * mp + 255) / 256)), dim3(256), 0, ctx->stream, ptr, ci, val, V, n_rows, mp, mpp, Np, Mt);
}

extern "C" int asb_rforce_operator(asb_ctx* ctx, int64_t n_rows, const int64_t* indptr, const int64_t* indices, const double* data,
                                   int64_t v_rows, int64_t mp, const double* V) {
    if (!ctx || !indptr || !V || n_rows < 1) return ASB_ERR_ARG;
    asb_ctx::RfBank& b = asb_rf_cur(ctx);
    b.mp = 0, b.r = 0, b.ok = 0, b.zok = 0;                    // this bank's operator, solver and A^-1 S^T V mark; no other bank's
    if (!ctx->X || ctx->v0 != 0 || ctx->n_loc != ctx->N_glob)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_rforce_operator: no whole tensor on the device (one rank only)");
    if (n_rows != ctx->n_loc)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_rforce_operator: S^T has %lld rows, the tensor %lld vertices", (long long)n_rows, (long long)ctx->n_loc);
    if (v_rows < 1 || mp < 1) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_rforce_operator: a basis of %lld rows x %lld vectors", (long long)v_rows, (long long)mp);
    const long long mpp = (mp + 3) / 4 * 4, Np = (n_rows + RF_TN - 1) / RF_TN * RF_TN;
    if (mp > 0x7fffffffLL / 4 || v_rows * mp > 0x7fffffffLL || n_rows * mp > 0x7fffffffLL * 256LL)
        ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_rforce_operator: %lld x %lld basis, %lld vertices: too large for 32-bit indices", (long long)v_rows,
                 (long long)mp, (long long)n_rows);
    std::vector<int> p32, c32;
    int rc;
    if ((rc = asb_csr_check32(ctx, "asb_rforce_operator", n_rows, indptr, indices, data, v_rows, p32, c32))) return rc;
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    asb_tmp<int> dptr, dci;
    asb_tmp<double> dval, dV;
    if ((rc = dptr.alloc(ctx, p32.size()))) return rc;
    if ((rc = dci.alloc(ctx, c32.size() + 1))) return rc;
    if ((rc = dval.alloc(ctx, c32.size() + 1))) return rc;
    if ((rc = dV.alloc(ctx, (size_t)v_rows * mp * 3))) return rc;
    if ((rc = asb_alloc(ctx, &b.M, (size_t)3 * mpp * Np))) return rc;
    if ((rc = asb_csr_stage(ctx, p32, c32, data, dptr.get(), dci.get(), dval.get()))) return rc;
    ASB_HIP(ctx, hipMemcpyAsync(dV.get(), V, (size_t)v_rows * mp * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemsetAsync(b.M, 0, (size_t)3 * mpp * Np * sizeof(double), ctx->stream));
    const unsigned grid = (unsigned)((n_rows * mp + 255) / 256);
    hipLaunchKernelGGL(k_st_dense, dim3(grid), dim3(256), 0, ctx->stream, dptr.get(), dci.get(), dval.get(), dV.get(), (long long)n_rows,
                       (int)mp, (int)mpp, Np, b.M);
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));          // the staging vectors and the temporaries die here
    b.n = n_rows, b.Np = Np, b.mp = mp, b.mpp = mpp;
    return ASB_OK;
}

extern "C" int asb_rforce_solver(asb_ctx* ctx, int64_t r, int64_t npt, const double* H, const int64_t* rows) {
    if (!ctx || !H || !rows) return ASB_ERR_ARG;
    asb_ctx::RfBank& b = asb_rf_cur(ctx);
    b.r = 0;
    if (b.mp < 1) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_rforce_solver: no operator on the device (asb_rforce_operator)");
    if (r < 1 || r > b.mp)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_rforce_solver: %lld basis vectors, the operator has %lld", (long long)r, (long long)b.mp);
    if (r > 65532) ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_rforce_solver: %lld basis vectors (at most 65532)", (long long)r);
    if (npt < 1 || npt > 0x7fffffffLL / r) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_rforce_solver: %lld interpolation rows", (long long)npt);
    std::vector<int> r32((size_t)npt);
    int64_t mx = -1;
    for (int64_t t = 0; t < npt; ++t) {
        if (rows[t] < 0 || rows[t] > 0x7fffffffLL / 4)
            ASB_FAIL(ctx, ASB_ERR_ARG, "asb_rforce_solver: interpolation point %lld names row %lld", (long long)t, (long long)rows[t]);
        r32[t] = (int)rows[t];
        if (rows[t] > mx) mx = rows[t];
    }
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    int rc;
    if ((rc = asb_alloc(ctx, &b.H, (size_t)3 * r * npt))) return rc;
    if ((rc = asb_alloc(ctx, &b.pt, (size_t)npt))) return rc;
    ASB_HIP(ctx, hipMemcpyAsync(b.H, H, (size_t)3 * r * npt * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemcpyAsync(b.pt, r32.data(), (size_t)npt * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));          // (the staging vector dies here)
    b.r = r, b.npt = npt, b.pt_max = mx;
    return ASB_OK;
}

// ---------------------------------------------------------------- the banks
// Held per bank, in ctx->rf_bank[bank] and nowhere else: S^T V (M), H and its rows (H, pt), the coefficients of one chunk
// (coef), A^-1 S^T V with its mark (G, ok) and its touched columns (Gc).  A selection is the index rf_cur: no buffer and no
// number moves, a bank that was addressed keeps what it holds whichever bank is current, and one never addressed holds nothing.
void asb_rf_invalidate_all(asb_ctx* ctx) {
    for (int k = 0; k < ASB_RFORCE_BANKS; ++k) ctx->rf_bank[k].ok = ctx->rf_bank[k].zok = 0;
}

extern "C" int asb_rforce_bank(asb_ctx* ctx, int bank) {
    if (!ctx) return ASB_ERR_ARG;
    if (bank < 0 || bank >= ASB_RFORCE_BANKS) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_rforce_bank: bank %d of 0..%d", bank, ASB_RFORCE_BANKS - 1);
    ctx->rf_cur = bank;
    return ASB_OK;
}

// whole frame tiles of the product, the scratch (projections + coefficients) within RF_SCRATCH_BYTES
long long asb_rforce_chunk_width(long long r, long long n_cols, long long n_sel) {
    const int rpp = ((int)r + 3) / 4 * 4;
    long long cw = (long long)(RF_SCRATCH_BYTES / (24ull * (unsigned long long)(n_cols + rpp)));
    cw = cw >= RF_TF ? cw / RF_TF * RF_TF : RF_TF;
    const long long span = (n_sel + RF_TF - 1) / RF_TF * RF_TF;
    return cw > span ? span : cw;
}

void asb_rforce_coef_launch(asb_ctx* ctx, const asb_ctx::RfBank& v, const double* S, int cw, int cn) {
    const int r = (int)v.r, rpp = (r + 3) / 4 * 4, npt = (int)v.npt;
    hipLaunchKernelGGL(k_rforce_coef, dim3((unsigned)(cw / 64), (unsigned)rpp, 3), dim3(64), 0, ctx->stream, v.H, v.pt, r, npt, rpp, S, cw, cn,
                       v.coef);
}

void asb_rforce_chunk_launch(asb_ctx* ctx, const asb_ctx::RfBank& v, const double* S, int cw, int c0, int cn, int accumulate, double* out) {
    const int rpp = ((int)v.r + 3) / 4 * 4;
    asb_rforce_coef_launch(ctx, v, S, cw, cn);
    hipLaunchKernelGGL(k_rforce_gemm, dim3((unsigned)(v.Np / RF_TN), (unsigned)((cn + RF_TF - 1) / RF_TF)), dim3(256), 0, ctx->stream, v.M,
                       (long long)v.Np, (int)v.mpp, v.coef, cw, rpp, c0, cn, (long long)v.n, accumulate ? 1 : 0, out);
}

extern "C" int asb_rforce_run(asb_ctx* ctx, int which, int64_t f0, int64_t f1, int64_t fj, const double* inv_massL, int add_mean, double psf,
                              double sigma_min, double sigma_max, int accumulate, double* out_dev) {
    if (!ctx || !out_dev) return ASB_ERR_ARG;
    CpWorld w;
    int64_t n_sel;
    int rc;
    if ((rc = asb_cproj_world(ctx, "asb_rforce_run", which, f0, f1, fj, add_mean, psf, sigma_min, sigma_max, &w, &n_sel))) return rc;
    asb_ctx::RfBank& b = asb_rf_cur(ctx);
    if (b.mp < 1 || b.r < 1) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_rforce_run: no operator or solver on the device (asb_rforce_operator, asb_rforce_solver)");
    if (b.n != ctx->n_loc)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_rforce_run: the operator has %lld rows, the tensor %lld vertices", (long long)b.n, (long long)ctx->n_loc);
    const long long n_cols = asb_cproj_rows(ctx->cp.kind, ctx->cp.n);
    if (b.pt_max >= n_cols)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_rforce_run: an interpolation point names row %lld, the sampled elements have %lld", (long long)b.pt_max, n_cols);
    const int rpp = ((int)b.r + 3) / 4 * 4;
    const long long cw = asb_rforce_chunk_width(b.r, n_cols, n_sel);
    if ((rc = asb_cproj_invm(ctx, inv_massL, &w))) return rc;
    if ((rc = asb_alloc(ctx, &ctx->cf_scratch, (size_t)3 * n_cols * cw))) return rc;
    if ((rc = asb_alloc(ctx, &b.coef, (size_t)3 * rpp * cw))) return rc;
    for (long long c0 = 0; c0 < n_sel; c0 += cw) {
        const int cn = (int)(c0 + cw < n_sel ? cw : n_sel - c0);
        asb_cproj_em_launch(ctx, ctx->cp, w, (int)f0, (int)fj, (int)c0, cn, (int)cw, sigma_min, sigma_max, ctx->cf_scratch);
        asb_rforce_chunk_launch(ctx, b, ctx->cf_scratch, (int)cw, (int)c0, cn, accumulate, out_dev);
    }
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));          // the caller owns out_dev and may read it on any stream
    return ASB_OK;
}

// ---------------------------------------------------------------- the error of b against a
// record of one frame / of all (FD_REC, fd_combine: asb_common.h): [0..2] sum (a - b)^2 per axis, [3..5] sum a^2 per axis,
// [6] max |a - b|, [7] max a

// the block's 256 records -> thread 0's, by a fixed tree
__device__ __forceinline__ void fd_block_reduce(double (&x)[FD_REC], double* sm) {
#pragma unroll
    for (int q = 0; q < FD_REC; ++q) sm[threadIdx.x * FD_REC + q] = x[q];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            fd_combine(x, sm + (threadIdx.x + s) * FD_REC);
#pragma unroll
            for (int q = 0; q < FD_REC; ++q) sm[threadIdx.x * FD_REC + q] = x[q];
        }
        __syncthreads();
    }
}

// grid (frames): part[f] = the record of frame f
__global__ __launch_bounds__(256) void k_force_diff(const double* __restrict__ a, const double* __restrict__ b, long long n_verts,
                                                    double* __restrict__ part) {
    __shared__ double sm[256 * FD_REC];
    const double* pa = a + (long long)blockIdx.x * n_verts * 3;
    const double* pb = b + (long long)blockIdx.x * n_verts * 3;
    double x[FD_REC] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -INFINITY};
    for (long long v = threadIdx.x; v < n_verts; v += 256) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double av = pa[3 * v + d], e = av - pb[3 * v + d];
            x[d] = fma(e, e, x[d]);
            x[3 + d] = fma(av, av, x[3 + d]);
            x[6] = fmax(x[6], fabs(e));
            x[7] = fmax(x[7], av);
        }
    }
    fd_block_reduce(x, sm);
    if (threadIdx.x == 0)
#pragma unroll
        for (int q = 0; q < FD_REC; ++q) part[(long long)blockIdx.x * FD_REC + q] = x[q];
}

// one block: part[F] = the records of the frames combined (thread t takes frames t, t + 256, .. in order, then the tree)
__global__ __launch_bounds__(256) void k_force_diff_final(double* __restrict__ part, long long F) {
    __shared__ double sm[256 * FD_REC];
    double x[FD_REC] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -INFINITY};
    for (long long f = threadIdx.x; f < F; f += 256) fd_combine(x, part + f * FD_REC);
    fd_block_reduce(x, sm);
    if (threadIdx.x == 0)
#pragma unroll
        for (int q = 0; q < FD_REC; ++q) part[F * FD_REC + q] = x[q];
}

extern "C" int asb_force_diff(asb_ctx* ctx, const double* a_dev, const double* b_dev, int64_t F, int64_t N, double* sums_out, double* max_out,
                              double* norms_out, double* per_frame_out) {
    if (!ctx || !a_dev || !b_dev) return ASB_ERR_ARG;
    if (F < 1 || N < 1 || F > 0x7fffffffLL) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_force_diff: tensors of %lld frames x %lld vertices", (long long)F, (long long)N);
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    int rc;
    if ((rc = asb_alloc(ctx, &ctx->fd_part, (size_t)(F + 1) * FD_REC))) return rc;
    hipLaunchKernelGGL(k_force_diff, dim3((unsigned)F), dim3(256), 0, ctx->stream, a_dev, b_dev, (long long)N, ctx->fd_part);
    asb_force_diff_final_launch(ctx, ctx->fd_part, (long long)F);
    ASB_CHECK_LAUNCH(ctx);
    return asb_force_diff_outputs(ctx, ctx->fd_part, (long long)F, sums_out, max_out, norms_out, per_frame_out);
}

void asb_force_diff_final_launch(asb_ctx* ctx, double* rec, long long F) {
    hipLaunchKernelGGL(k_force_diff_final, dim3(1), dim3(256), 0, ctx->stream, rec, F);
}

int asb_force_diff_outputs(asb_ctx* ctx, const double* rec_dev, long long F, double* sums_out, double* max_out, double* norms_out,
                           double* per_frame_out) {
    std::vector<double> rec((size_t)(F + 1) * FD_REC);
    const size_t skip = per_frame_out ? 0 : (size_t)F * FD_REC;
    ASB_HIP(ctx, hipMemcpyAsync(rec.data() + skip, rec_dev + skip, (rec.size() - skip) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const double* tot = rec.data() + (size_t)F * FD_REC;
    if (sums_out) sums_out[0] = tot[0], sums_out[1] = tot[1], sums_out[2] = tot[2];
    if (norms_out) norms_out[0] = tot[3], norms_out[1] = tot[4], norms_out[2] = tot[5], norms_out[3] = tot[7];
    if (max_out) max_out[0] = tot[6];
    if (per_frame_out)
        for (long long f = 0; f < F; ++f) {
            const double* x = rec.data() + (size_t)f * FD_REC;
            per_frame_out[2 * f] = x[0] + x[1] + x[2];
            per_frame_out[2 * f + 1] = x[3] + x[4] + x[5];
        }
    return ASB_OK;
}
