// The global step's third solver: the step restricted to a POSITION SUBSPACE q = o + U z (the reference's `reduced_position`
// branch, projective_dynamics/Simulators.py:38-41, :144-155, :195, :239, which it leaves unimplemented).  Per coordinate d, for a
// basis U_d (N x r) of full column rank and an origin o (N x 3), the Galerkin step is
//   q_d = o_d + U_d (U_d^T A U_d)^-1 U_d^T (rhs_d - A o_d)  =  o'_d + P_d rhs_d,     P_d = U_d At_d^-1 U_d^T,  o'_d = o_d - P_d A o_d,
// affine in the right-hand side: a third holder behind everything that dispatches on "inverse or slab factor".
//
//   asb_gsub_setup    the host CSR of A_N with the checks of asb_gstep_setup, U_d^T as (3, r, n) (the host has orthonormalised
//                     it: projections.subspace_basis) and o.  U^T is uploaded in the operator layout (3, rp, Np) (rp = r rounded
//                     up to 4, Np = N to 32, zero padding: RfBank::M's), A U_d comes from k_st_dense (asb_rforce.hip), At_d = U_d^T (A U_d)
//                     from asb_gemm_tn_s, padded to rq = r rounded up to 16 by an identity block and inverted by asb_dense_spd_inverse
//                     (not positive definite: that call's error, no solver is left), W_d^T = U_d At_d^-1 from asb_gemm_nn, kept
//                     vertex by vertex as (3, Np, rq).  o' and the residual max_d max |U_d^T (A (P_d 1) - 1)| are formed with the
//                     two product kernels below on a work matrix of two columns.  The context then holds exactly one of
//                     inverse / factor / subspace.
//   k_gsub_reduce     Y_d (rq x ld) = W_d (rq x N) R_d (N x ld), R_d the rows 3 v + d of the vertex-major work matrix R (3 Np, ld):
//                     v_mfma_f64_16x16x4_f64 with A = W (j x vertices) and B = R (vertices x frames).  A block of 4 waves owns
//                     up to 64 rows j x 64 frames (wave w: frames 16 w .., up to four accumulators that share the B operand)
//                     and walks ALL N in ascending order: the contraction is never split between blocks, an entry of Y is one
//                     accumulator from zero.  W is stored (Np, rq): the 16 lanes of an A load read 16 consecutive doubles, as
//                     those of a B load do.  W's rows past N are zero and R has 3 Np rows (its padding zero): no load carries a
//                     bounds predicate -- the only condition is block-uniform, the number of 16-row tiles of j.  No atomics.
//   k_gsub_expand     Q[3 v + d][f] = fl(o'[v][d] affine + sum_j U_d[v][j] Y_d[j][f]), j ascending from a zero accumulator: the
//                     roles and the store pattern of k_hyper_apply (A = vertices x j, B = j x frames; asb_pdsolve.hip), a block
//                     of 4 waves owns 32 vertices x 64 frames x 3 coordinates, stores are direct 128-byte runs into Q.  FM: the
//                     same values are also staged frame-major through LDS rows of 97 doubles and written per frame as runs of 96.
//                     Tail predicates: vertices >= n, frames >= F; the padding columns of Q are never written.
// An entry's value does not depend on the tile, chunk or row set it falls in, nor on the columns beside it.
// The frame-major input goes through k_pd_transpose (asb_pdsolve.hip) into R; asb_gsub_solve_rows (the LINEAR part P_d M_d, for
// G of asb_hyper_operator) moves the rows of an operator in and out with k_gsub_rows.
#include "asb_common.h"

#include <algorithm>
#include <cmath>
#include <vector>

typedef double gb_d4 __attribute__((ext_vector_type(4)));

#define GB_MAX_R 8192       // the largest subspace: three dense r x r inverses
#define GB_TF 64            // frames per block of both kernels (16 per wave)
#define GB_TJ 64            // rows of Y per block of k_gsub_reduce (four tiles of 16)
#define GB_TN 32            // vertices per block of k_gsub_expand
#define GB_KS 8             // steps of 4 vertices per trip of k_gsub_reduce's loop: Np is a multiple of 32

struct asb_gsb {
    long long n = 0, r = 0, rp = 0, rq = 0, Np = 0;   // vertices (0: no subspace), basis vectors, rounded up to 4 and 16; N to 32
    double *Ut = nullptr, *Wn = nullptr, *Ai = nullptr, *op = nullptr;    // (3, rp, Np), (3, Np, rq), (3, rq, rq), (n, 3)
    double *R = nullptr, *Y = nullptr, *V = nullptr;  // work matrix (3 Np, ld), (3, rq, ld), vertex-major result of asb_gstep_run
    double *Un = nullptr, *o = nullptr, *Ao = nullptr;        // for asb_zroll.hip: U in W's layout (3, Np, rq), the origin (n, 3), A o (n, 3)
    const double* R_at = nullptr;                     // the R whose padding is known to be zero for rows of R_ld doubles
    long long R_ld = 0;
    long long gen = 0;                                // which set-up this is: asb_zroll.hip refuses what another one formed
};

long long asb_gsub_n(const asb_ctx* ctx) { return ctx->gsb ? ctx->gsb->n : 0; }

void asb_gsub_release(asb_ctx* ctx) {
    asb_gsb* s = ctx->gsb;
    if (!s) return;
    s->n = 0, s->R_at = nullptr;
    (void)asb_alloc(ctx, &s->Ut, 0), (void)asb_alloc(ctx, &s->Wn, 0), (void)asb_alloc(ctx, &s->Ai, 0), (void)asb_alloc(ctx, &s->op, 0);
    (void)asb_alloc(ctx, &s->R, 0), (void)asb_alloc(ctx, &s->Y, 0), (void)asb_alloc(ctx, &s->V, 0);
    (void)asb_alloc(ctx, &s->Un, 0), (void)asb_alloc(ctx, &s->o, 0), (void)asb_alloc(ctx, &s->Ao, 0);
}

void asb_gsub_free(asb_ctx* ctx) {                // (the buffers went with the context's registered allocations)
    delete ctx->gsb;
    ctx->gsb = nullptr;
}

// ---------------------------------------------------------------- the two products
// grid (ld / 64, blocks of 16 NJ rows from row jb, 3); Wn (3, Np, rq); R (3 Np, ld); Y (3, rq, ld).  Np a multiple of 32, rq of 16,
// ld of 64.  NJ: the 16-row tiles of Y a wave carries (4 for the full blocks, the remainder in a launch of its own): an entry's
// chain of MFMAs is the same under every NJ
template <int NJ>
__global__ __launch_bounds__(256) void k_gsub_reduce(const double* __restrict__ Wn, long long Np, int rq, int jb, const double* __restrict__ R,
                                                     long long ld, double* __restrict__ Y) {
    const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int d = blockIdx.z, j0 = jb + (int)blockIdx.y * 16 * NJ;
    const long long f = (long long)blockIdx.x * GB_TF + wave * 16 + i;
    gb_d4 acc[NJ];
#pragma unroll
    for (int t = 0; t < NJ; ++t) acc[t] = gb_d4{0.0, 0.0, 0.0, 0.0};
    const double* pa = Wn + ((long long)d * Np + g) * rq + j0 + i;    // A: row j0 + 16 t + i, k = vertex k0 + g
    const double* pb = R + (3LL * g + d) * ld + f;                     // B: k = vertex k0 + g, frame f
    for (long long k0 = 0; k0 < Np; k0 += 4 * GB_KS) {                 // GB_KS steps of 4 per trip: all their loads are issued together
        double b[GB_KS], a[GB_KS][NJ];
#pragma unroll
        for (int s = 0; s < GB_KS; ++s) {
            b[s] = pb[3 * (k0 + 4 * s) * ld];
#pragma unroll
            for (int t = 0; t < NJ; ++t) a[s][t] = pa[(k0 + 4 * s) * rq + 16 * t];
        }
#pragma unroll
        for (int s = 0; s < GB_KS; ++s)                                // ascending k: the order of an entry's chain is fixed
#pragma unroll
            for (int t = 0; t < NJ; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s][t], b[s], acc[t], 0, 0, 0);
    }
    // accumulator q of lane (i, g): row g + 4 q of the tile's 16, frame i of the wave's 16
#pragma unroll
    for (int t = 0; t < NJ; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) Y[((long long)d * rq + j0 + 16 * t + g + 4 * q) * ld + f] = acc[t][q];
}

static void gsb_reduce_launch(asb_ctx* ctx, const double* Wn, long long Np, int rq, const double* R, long long ld, double* Y) {
    const unsigned gx = (unsigned)(ld / GB_TF);
    const int full = rq / GB_TJ, rest = (rq % GB_TJ) / 16;
    if (full) hipLaunchKernelGGL(k_gsub_reduce<4>, dim3(gx, (unsigned)full, 3), dim3(256), 0, ctx->stream, Wn, Np, rq, 0, R, ld, Y);
    const int jb = full * GB_TJ;
    if (rest == 1) hipLaunchKernelGGL(k_gsub_reduce<1>, dim3(gx, 1, 3), dim3(256), 0, ctx->stream, Wn, Np, rq, jb, R, ld, Y);
    if (rest == 2) hipLaunchKernelGGL(k_gsub_reduce<2>, dim3(gx, 1, 3), dim3(256), 0, ctx->stream, Wn, Np, rq, jb, R, ld, Y);
    if (rest == 3) hipLaunchKernelGGL(k_gsub_reduce<3>, dim3(gx, 1, 3), dim3(256), 0, ctx->stream, Wn, Np, rq, jb, R, ld, Y);
}

// grid (Np / 32, ld / 64); Ut (3, rp, Np); Y (3, rq, ld); op (n, 3); Q (3 n, ld); out (F, n, 3) with FM.  affine 1: o' is added, 0: not
template <bool FM>
__global__ __launch_bounds__(256) void k_gsub_expand(const double* __restrict__ Ut, long long Np, int rp, const double* __restrict__ Y, int rq,
                                                     long long ld, const double* __restrict__ op, int affine, double* __restrict__ Q, int F,
                                                     int n, double* __restrict__ out) {
    constexpr int RUN = GB_TN * 3, ROW = RUN + 1;
    __shared__ double stage[FM ? GB_TF * ROW : 1];
    const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int v0 = (int)blockIdx.x * GB_TN;
    const int t0 = (int)blockIdx.y * GB_TF;
    gb_d4 acc[3][2];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[d][y] = gb_d4{0.0, 0.0, 0.0, 0.0};
    const double* pa = Ut + v0 + i;                                   // A: vertex i of 16, k = g
    const double* pb = Y + t0 + wave * 16 + i;                        // B: k = g, frame i of the wave's 16
    for (int k0 = 0; k0 < rp; k0 += 4) {
        const int k = k0 + g;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double* a = pa + ((long long)d * rp + k) * Np;
            const double b = pb[((long long)d * rq + k) * ld];
            acc[d][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0], b, acc[d][0], 0, 0, 0);
            acc[d][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[16], b, acc[d][1], 0, 0, 0);
        }
    }
    // accumulator q of lane (i, g): vertex g + 4 q of the 16, frame i of the wave's 16
    const int fl = wave * 16 + i;
    const bool fok = t0 + fl < F;
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int vl = 16 * y + g + 4 * q;
                double val = 0.0;
                if (fok && v0 + vl < n) {
                    const long long row = 3LL * (v0 + vl) + d;
                    const double base = affine ? op[row] : 0.0;
                    val = base + acc[d][y][q];
                    Q[row * ld + t0 + fl] = val;
                }
                if (FM) stage[fl * ROW + vl * 3 + d] = val;
            }
    if (FM) {
        __syncthreads();
        const int nvt = n - v0 < GB_TN ? n - v0 : GB_TN;
        const int nf = F - t0 < GB_TF ? F - t0 : GB_TF;
        const int run = nvt * 3;
        for (int e = threadIdx.x; e < GB_TF * RUN; e += 256) {
            const int fr = e / RUN, k = e % RUN;
            if (fr < nf && k < run) out[((long long)(t0 + fr) * n + v0) * 3 + k] = stage[fr * ROW + k];
        }
    }
}

// grid (blocks of 256 over n, rows = 3 mpp): row d mpp + j of an operator (rows, Np), vertices contiguous, <-> column j of row
// 3 v + d of a vertex-major matrix (row length ld).  IN: into the work matrix; otherwise back into the operator's layout
// (the operator's side is read / written in 2 KB runs, the vertex-major side one double per thread at stride 3 ld: uncoalesced,
// accepted for a path that runs once per operator; the rows sit on grid.y, hence at most 65 535 of them, mpp <= 21 845)
template <bool IN>
__global__ __launch_bounds__(256) void k_gsub_rows(double* __restrict__ Mt, long long Np, int mpp, double* __restrict__ Vm, long long ld, int n) {
    const int v = (int)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const int d = (int)blockIdx.y / mpp, j = (int)blockIdx.y % mpp;
    double* m = Mt + (long long)blockIdx.y * Np + v;
    double* x = Vm + (3LL * v + d) * ld + j;
    if (IN) *x = *m;
    else *m = *x;
}

// ---------------------------------------------------------------- the set-up's small kernels (blocks of 256 over 3 n entries)
// At (rq x rq): the identity block of the padding
__global__ __launch_bounds__(256) void k_gsub_eye(double* __restrict__ At, int r, int rq) {
    const int k = r + (int)blockIdx.x * 256 + threadIdx.x;
    if (k < rq) At[(long long)k * rq + k] = 1.0;
}
// columns 0 and 1 of the work matrix: (A o)_d, from k_st_dense's (3, 4, Np), and 1
__global__ __launch_bounds__(256) void k_gsub_cols(const double* __restrict__ AoT, long long Np, int n, double* __restrict__ R, long long ld) {
    const int e = (int)blockIdx.x * 256 + threadIdx.x;
    if (e >= 3 * n) return;
    const int v = e / 3, d = e % 3;
    R[(long long)e * ld] = AoT[(4LL * d) * Np + v];
    R[(long long)e * ld + 1] = 1.0;
}
// o' = o - P A o (column 0 of Qv) and x = P 1 (column 1), the latter as k_st_dense's basis of one vector (n, 1, 3)
__global__ __launch_bounds__(256) void k_gsub_origin(const double* __restrict__ o, const double* __restrict__ Qv, long long ld, int n,
                                                     double* __restrict__ op, double* __restrict__ xs) {
    const int e = (int)blockIdx.x * 256 + threadIdx.x;
    if (e >= 3 * n) return;
    op[e] = o[e] - Qv[(long long)e * ld];
    xs[e] = Qv[(long long)e * ld + 1];
}
// column 0 of the work matrix: (A x)_d - 1
__global__ __launch_bounds__(256) void k_gsub_rcol(const double* __restrict__ AxT, long long Np, int n, double* __restrict__ R, long long ld) {
    const int e = (int)blockIdx.x * 256 + threadIdx.x;
    if (e >= 3 * n) return;
    R[(long long)e * ld] = AxT[(4LL * (e % 3)) * Np + e / 3] - 1.0;
}

// ---------------------------------------------------------------- applying the map
// the work matrices for rows of ld doubles; R's padding (rows past 3 n, and everything of a new buffer) is zero afterwards
static int gsb_work(asb_ctx* ctx, asb_gsb* s, long long ld) {
    int rc;
    if ((rc = asb_alloc(ctx, &s->R, (size_t)3 * s->Np * ld))) return rc;
    if ((rc = asb_alloc(ctx, &s->Y, (size_t)3 * s->rq * ld))) return rc;
    if (s->R_at != s->R || s->R_ld != ld) {
        ASB_HIP(ctx, hipMemsetAsync(s->R, 0, (size_t)3 * s->Np * ld * sizeof(double), ctx->stream));
        s->R_at = s->R, s->R_ld = ld;
    }
    return ASB_OK;
}

// R (filled) -> Y -> Qv (3 n, ld), columns [0, F); out (optional): the same values frame-major (F, n, 3)
static void gsb_apply(asb_ctx* ctx, const asb_gsb* s, const double* Wn, long long ld, long long F, int affine, double* Qv, double* out) {
    gsb_reduce_launch(ctx, Wn, s->Np, (int)s->rq, s->R, ld, s->Y);
    if (!Qv) return;
    const dim3 ge((unsigned)(s->Np / GB_TN), (unsigned)(ld / GB_TF));
    if (out)
        hipLaunchKernelGGL((k_gsub_expand<true>), ge, dim3(256), 0, ctx->stream, s->Ut, s->Np, (int)s->rp, s->Y, (int)s->rq, ld, s->op, affine, Qv,
                           (int)F, (int)s->n, out);
    else
        hipLaunchKernelGGL((k_gsub_expand<false>), ge, dim3(256), 0, ctx->stream, s->Ut, s->Np, (int)s->rp, s->Y, (int)s->rq, ld, s->op, affine, Qv,
                           (int)F, (int)s->n, nullptr);
}

int asb_gsub_solve_fm(asb_ctx* ctx, const double* rhs, long long F, double* Qv, double* out) {
    asb_gsb* s = ctx->gsb;
    if (!s || s->n < 1) ASB_FAIL(ctx, ASB_ERR_ARG, "no position subspace on the device (asb_gsub_setup)");
    const long long ld = (F + 63) / 64 * 64;
    int rc;
    if ((rc = gsb_work(ctx, s, ld))) return rc;
    if (!Qv) {
        if ((rc = asb_alloc(ctx, &s->V, (size_t)3 * s->n * ld))) return rc;
        Qv = s->V;
    }
    asb_pd_transpose_launch(ctx, rhs, (int)F, 3 * s->n, s->R, ld);
    gsb_apply(ctx, s, s->Wn, ld, F, 1, Qv, out);
    ASB_CHECK_LAUNCH(ctx);
    return ASB_OK;
}

int asb_gsub_solve_rows(asb_ctx* ctx, const double* Mt, long long rows, long long Np, double* Ot) {
    asb_gsb* s = ctx->gsb;
    if (!s || s->n < 1) ASB_FAIL(ctx, ASB_ERR_ARG, "no position subspace on the device (asb_gsub_setup)");
    if (Np != s->Np || rows < 3 || rows % 3 || rows > 65535)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_gsub_solve_rows: an operator of %lld rows of %lld doubles (the subspace pads to %lld)", rows, Np, s->Np);
    const long long mpp = rows / 3, ld = (mpp + 63) / 64 * 64;
    asb_tmp<double> Qv;                             // (3 n, ld): the vertices' rows, the columns of the solve contiguous
    int rc;
    if ((rc = gsb_work(ctx, s, ld))) return rc;
    if ((rc = Qv.alloc(ctx, (size_t)3 * s->n * ld))) return rc;
    const dim3 gr((unsigned)((s->n + 255) / 256), (unsigned)rows);
    hipLaunchKernelGGL(k_gsub_rows<true>, gr, dim3(256), 0, ctx->stream, const_cast<double*>(Mt), Np, (int)mpp, s->R, ld, (int)s->n);
    gsb_apply(ctx, s, s->Wn, ld, mpp, 0, Qv.get(), nullptr);
    hipLaunchKernelGGL(k_gsub_rows<false>, gr, dim3(256), 0, ctx->stream, Ot, Np, (int)mpp, Qv.get(), ld, (int)s->n);
    ASB_CHECK_LAUNCH(ctx);
    return ASB_OK;
}

// ---------------------------------------------------------------- what asb_zroll.hip takes from this unit
int asb_gsub_view(asb_ctx* ctx, GsubView* v) {
    const asb_gsb* s = ctx->gsb;
    if (!s || s->n < 1) return 0;
    *v = GsubView{s->n, s->r, s->rp, s->rq, s->Np, s->gen, s->Ut, s->Wn, s->Un, s->o, s->Ao};
    return 1;
}

int asb_gsub_work(asb_ctx* ctx, long long ld, double** R, double** Y) {
    asb_gsb* s = ctx->gsb;
    int rc;
    if ((rc = gsb_work(ctx, s, ld))) return rc;
    *R = s->R, *Y = s->Y;
    return ASB_OK;
}

void asb_gsub_reduce_launch(asb_ctx* ctx, int basis, long long ld, double* Y) {
    const asb_gsb* s = ctx->gsb;
    gsb_reduce_launch(ctx, basis ? s->Un : s->Wn, s->Np, (int)s->rq, s->R, ld, Y);
}

void asb_gsub_expand_launch(asb_ctx* ctx, const double* Ut, long long Np, const double* Y, long long ld, const double* base, double* Q,
                            long long F, long long n, double* out) {
    const asb_gsb* s = ctx->gsb;
    const dim3 ge((unsigned)(Np / GB_TN), (unsigned)(ld / GB_TF));
    if (out)
        hipLaunchKernelGGL((k_gsub_expand<true>), ge, dim3(256), 0, ctx->stream, Ut, Np, (int)s->rp, Y, (int)s->rq, ld, base, 1, Q, (int)F, (int)n, out);
    else
        hipLaunchKernelGGL((k_gsub_expand<false>), ge, dim3(256), 0, ctx->stream, Ut, Np, (int)s->rp, Y, (int)s->rq, ld, base, 1, Q, (int)F, (int)n,
                           nullptr);
}

int asb_gsub_rows_in(asb_ctx* ctx, const double* Mt, long long rows, long long Np, long long* ld_out, double** Y) {
    asb_gsb* s = ctx->gsb;
    if (Np != s->Np || rows < 3 || rows % 3 || rows > 65535)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_operator: an operator of %lld rows of %lld doubles (the subspace pads to %lld)", rows, Np, s->Np);
    const long long mpp = rows / 3, ld = (mpp + 63) / 64 * 64;
    int rc;
    if ((rc = gsb_work(ctx, s, ld))) return rc;
    const dim3 gr((unsigned)((s->n + 255) / 256), (unsigned)rows);
    hipLaunchKernelGGL(k_gsub_rows<true>, gr, dim3(256), 0, ctx->stream, const_cast<double*>(Mt), Np, (int)mpp, s->R, ld, (int)s->n);
    gsb_reduce_launch(ctx, s->Wn, s->Np, (int)s->rq, s->R, ld, s->Y);
    *ld_out = ld, *Y = s->Y;
    return ASB_OK;
}

// ---------------------------------------------------------------- set-up
extern "C" int asb_gsub_setup(asb_ctx* ctx, int64_t n, const int64_t* indptr, const int64_t* indices, const double* data, int64_t r,
                              const double* Qt_host, const double* origin_host, double* resid_out) {
    if (!ctx || !indptr || !Qt_host || !origin_host || n < 1 || r < 1) return ASB_ERR_ARG;
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    // the context holds one solver: the explicit inverse goes, the slab factor, and an earlier subspace
    ctx->gs_n = 0;
    asb_rf_invalidate_all(ctx);
    (void)asb_alloc(ctx, &ctx->gs_Ainv, 0);
    asb_gslab_release(ctx);
    asb_gsub_release(ctx);
    if (r > n) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_gsub_setup: %lld basis vectors for %lld vertices", (long long)r, (long long)n);
    if (r > GB_MAX_R) ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_gsub_setup: %lld basis vectors (at most %d)", (long long)r, GB_MAX_R);
    if (n > 0x7fffffffLL / 4 - 32) ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_gsub_setup: %lld vertices do not fit 32-bit indices", (long long)n);
    std::vector<int> p32, c32;
    int rc;
    if ((rc = asb_gs_check_matrix(ctx, "asb_gsub_setup", n, indptr, indices, data, p32, c32))) return rc;
    for (int64_t e = 0; e < 3 * r * n; ++e)
        if (!std::isfinite(Qt_host[e])) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_gsub_setup: the basis holds a value that is not finite");
    for (int64_t e = 0; e < 3 * n; ++e)
        if (!std::isfinite(origin_host[e])) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_gsub_setup: the origin holds a value that is not finite");
    const long long rp = (r + 3) / 4 * 4, rq = (r + 15) / 16 * 16, Np = (n + 31) / 32 * 32;
    // ---- the three host layouts of the basis: U^T (3, rp, Np), U (3, Np, rq), and k_st_dense's (n, r, 3)
    std::vector<double> ut((size_t)3 * rp * Np, 0.0), un((size_t)3 * Np * rq, 0.0), uv((size_t)n * r * 3);
    for (int d = 0; d < 3; ++d)
        for (int64_t j = 0; j < r; ++j) {
            const double* q = Qt_host + ((size_t)d * r + j) * n;
            for (int64_t v = 0; v < n; ++v) {
                ut[((size_t)d * rp + j) * Np + v] = q[v];
                un[((size_t)d * Np + v) * rq + j] = q[v];
                uv[((size_t)v * r + j) * 3 + d] = q[v];
            }
        }
    if (!ctx->gsb) ctx->gsb = new asb_gsb();
    asb_gsb* s = ctx->gsb;
    static long long generation = 0;
    s->r = r, s->rp = rp, s->rq = rq, s->Np = Np, s->gen = ++generation;
    const long long ld = 64;
    if ((rc = asb_alloc(ctx, &s->Ut, ut.size()))) return rc;
    if ((rc = asb_alloc(ctx, &s->Wn, un.size()))) return rc;
    if ((rc = asb_alloc(ctx, &s->Ai, (size_t)3 * rq * rq))) return rc;
    if ((rc = asb_alloc(ctx, &s->op, (size_t)3 * n))) return rc;
    asb_tmp<int> dptr, dci;
    asb_tmp<double> dval, dV, AUt, AUn, Qv, xs;
    if ((rc = dptr.alloc(ctx, p32.size())) || (rc = dci.alloc(ctx, c32.size() + 1)) || (rc = dval.alloc(ctx, c32.size() + 1))) return rc;
    if ((rc = asb_alloc(ctx, &s->Un, un.size())) || (rc = dV.alloc(ctx, uv.size())) || (rc = AUt.alloc(ctx, (size_t)3 * std::max(rp, 4LL) * Np))) return rc;
    if ((rc = AUn.alloc(ctx, (size_t)Np * rp)) || (rc = asb_alloc(ctx, &s->o, (size_t)3 * n)) || (rc = Qv.alloc(ctx, (size_t)3 * n * ld))) return rc;
    if ((rc = xs.alloc(ctx, (size_t)3 * n)) || (rc = asb_alloc(ctx, &s->Ao, (size_t)3 * n))) return rc;
    if ((rc = asb_csr_stage(ctx, p32, c32, data, dptr.get(), dci.get(), dval.get()))) return rc;
    ASB_HIP(ctx, hipMemcpyAsync(s->Ut, ut.data(), ut.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemcpyAsync(s->Un, un.data(), un.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemcpyAsync(dV.get(), uv.data(), uv.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemcpyAsync(s->o, origin_host, (size_t)3 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    // ---- (A U_d)^T (3, rp, Np), then per coordinate At_d = U_d^T (A U_d), its inverse, W_d^T = U_d At_d^-1
    ASB_HIP(ctx, hipMemsetAsync(AUt.get(), 0, (size_t)3 * rp * Np * sizeof(double), ctx->stream));
    asb_st_dense_launch(ctx, dptr.get(), dci.get(), dval.get(), dV.get(), n, (int)r, (int)rp, Np, AUt.get());
    ASB_HIP(ctx, hipMemsetAsync(s->Ai, 0, (size_t)3 * rq * rq * sizeof(double), ctx->stream));
    ASB_CHECK_LAUNCH(ctx);
    for (int d = 0; d < 3; ++d) {
        double* At = s->Ai + (size_t)d * rq * rq;
        const double* Ud = s->Un + (size_t)d * Np * rq;
        if ((rc = asb_transpose(ctx, AUt.get() + (size_t)d * rp * Np, rp, Np, AUn.get()))) return rc;
        if ((rc = asb_gemm_tn_s(ctx, Ud, rq, 1, AUn.get(), rp, Np, (int)rp, (int)rp, At, rq, 1))) return rc;
        if (rq > r) hipLaunchKernelGGL(k_gsub_eye, dim3((unsigned)((rq - r + 255) / 256)), dim3(256), 0, ctx->stream, At, (int)r, (int)rq);
        ASB_CHECK_LAUNCH(ctx);
        if ((rc = asb_dense_spd_inverse(ctx, At, (int)rq))) return rc;        // (drains the stream: the host vectors may go after the first)
        if ((rc = asb_gemm_nn(ctx, Ud, rq, At, rq, s->Wn + (size_t)d * Np * rq, rq, (int)Np, (int)rq, (int)rq, 1.0, 0.0))) return rc;
    }
    // ---- o' = o - P A o and the residual U_d^T (A (P_d 1) - 1), through the two kernels on columns 0 and 1 of the work matrix
    s->n = n;                                       // (the products below read the holder; a failure takes it back)
    auto fail = [&](int code) { s->n = 0; return code; };
    if ((rc = gsb_work(ctx, s, ld))) return fail(rc);
    const unsigned g3 = (unsigned)((3 * n + 255) / 256);
    ASB_HIP(ctx, hipMemsetAsync(AUt.get(), 0, (size_t)3 * 4 * Np * sizeof(double), ctx->stream));
    asb_st_dense_launch(ctx, dptr.get(), dci.get(), dval.get(), s->o, n, 1, 4, Np, AUt.get());
    hipLaunchKernelGGL(k_gsub_cols, dim3(g3), dim3(256), 0, ctx->stream, AUt.get(), Np, (int)n, s->R, ld);
    ASB_HIP(ctx, hipMemcpy2DAsync(s->Ao, sizeof(double), s->R, (size_t)ld * sizeof(double), sizeof(double), (size_t)3 * n,      // column 0: A o, kept
                                  hipMemcpyDeviceToDevice, ctx->stream));
    gsb_apply(ctx, s, s->Wn, ld, 2, 0, Qv.get(), nullptr);
    hipLaunchKernelGGL(k_gsub_origin, dim3(g3), dim3(256), 0, ctx->stream, s->o, Qv.get(), ld, (int)n, s->op, xs.get());
    asb_st_dense_launch(ctx, dptr.get(), dci.get(), dval.get(), xs.get(), n, 1, 4, Np, AUt.get());
    hipLaunchKernelGGL(k_gsub_rcol, dim3(g3), dim3(256), 0, ctx->stream, AUt.get(), Np, (int)n, s->R, ld);
    gsb_apply(ctx, s, s->Un, ld, 1, 0, nullptr, nullptr);                  // Y = U^T (A x - 1): the basis in place of W
    if (hipGetLastError() != hipSuccess) return fail(ASB_ERR_HIP);
    std::vector<double> y((size_t)3 * rq * ld);
    if (hipMemcpyAsync(y.data(), s->Y, y.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) {                    // the staging vectors and the temporaries die here
        s->n = 0;
        ASB_FAIL(ctx, ASB_ERR_HIP, "asb_gsub_setup: the residual's copy failed");
    }
    double worst = 0.0;
    for (int d = 0; d < 3; ++d)
        for (int64_t j = 0; j < r; ++j) {
            const double e = std::fabs(y[((size_t)d * rq + j) * ld]);
            worst = (e > worst || e != e) ? e : worst;
        }
    if (resid_out) *resid_out = worst;
    return ASB_OK;
}

// counts_out (4): basis vectors r, r rounded up to 16 (rows of W and of the inverses), vertices rounded up to 32, r rounded up to 4
extern "C" int asb_gsub_info(asb_ctx* ctx, int64_t* counts_out) {
    if (!ctx || !counts_out) return ASB_ERR_ARG;
    const asb_gsb* s = ctx->gsb;
    if (!s || s->n < 1) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_gsub_info: no position subspace on the device (asb_gsub_setup)");
    counts_out[0] = s->r, counts_out[1] = s->rq, counts_out[2] = s->Np, counts_out[3] = s->rp;
    return ASB_OK;
}

// test hook: the map on a host matrix.  rhs_host (3 n, w) vertex-major, any w >= 1; out_host (3 n, ld), ld = w rounded up to 64, is
// read AND written: its columns [0, w) get o' affine + P rhs, the others come back as they went in
extern "C" int asb_test_gsub_apply(asb_ctx* ctx, const double* rhs_host, int64_t w, int affine, double* out_host) {
    if (!ctx || !rhs_host || !out_host || w < 1) return ASB_ERR_ARG;
    asb_gsb* s = ctx->gsb;
    if (!s || s->n < 1) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_test_gsub_apply: no position subspace on the device (asb_gsub_setup)");
    if (w > (1 << 22)) ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_test_gsub_apply: %lld columns", (long long)w);
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    const long long ld = (w + 63) / 64 * 64;
    asb_tmp<double> q;
    int rc;
    if ((rc = gsb_work(ctx, s, ld))) return rc;
    if ((rc = asb_test_stage(ctx, out_host, (size_t)3 * s->n * ld, 0, q))) return rc;
    ASB_HIP(ctx, hipMemcpy2DAsync(s->R, (size_t)ld * sizeof(double), rhs_host, (size_t)w * sizeof(double), (size_t)w * sizeof(double),
                                  (size_t)3 * s->n, hipMemcpyHostToDevice, ctx->stream));
    gsb_apply(ctx, s, s->Wn, ld, w, affine ? 1 : 0, q.get(), nullptr);
    rc = hipGetLastError() == hipSuccess ? ASB_OK : ASB_ERR_HIP;
    return asb_test_finish(ctx, rc, q.get(), out_host, (size_t)3 * s->n * ld);
}

// test hook: what the set-up left, as it lies on the device.  which 0: W^T (3, Np, rq); 1: the inverses (3, rq, rq); 2: o' (n, 3);
// 3: U^T (3, rp, Np).  len: the doubles of out_host, checked
extern "C" int asb_test_gsub_state(asb_ctx* ctx, int which, double* out_host, int64_t len) {
    if (!ctx || !out_host) return ASB_ERR_ARG;
    const asb_gsb* s = ctx->gsb;
    if (!s || s->n < 1) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_test_gsub_state: no position subspace on the device (asb_gsub_setup)");
    const double* src[4] = {s->Wn, s->Ai, s->op, s->Ut};
    const long long want[4] = {3 * s->Np * s->rq, 3 * s->rq * s->rq, 3 * s->n, 3 * s->rp * s->Np};
    if (which < 0 || which > 3 || len != want[which])
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_test_gsub_state: which %d with %lld doubles", which, (long long)len);
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    ASB_HIP(ctx, hipMemcpyAsync(out_host, src[which], (size_t)len * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ASB_OK;
}
