// Roll-outs of the hyper-reduced solver under the position subspace q = o + U z (asb_gsub.hip) with the STATE IN z: a time step
// touches r, the m_k of the reduced kinds, the P pins and the n_t touched vertices -- no pass over the N vertices is left in it.
// Per coordinate d, with At = U^T A U, W = At^-1 U^T, D = diag(masses / h^2), a = h^2 g and the origin o:
//   held per call    T = W D U (r x r),  kappa = W (D (o + a 1) - A o) (r),  E[:, i] = w_i W[:, v_i] (r x P, the pins),
//                    per bank Gz = W S^T V (r x m: asb_zroll_operator), the touched rows U_t (n_t x r) and o_t -- every one formed
//                    by the reduce Y = W R of asb_gsub.hip on a handful of columns: one chain over N per entry, never split
//   start            z_0 = U^T (x_f - o), z_-1 = U^T (x_{f-1} - o) (or z_0): the same reduce with U in place of W, once per call
//   step             y = fl(2 z - z_p), z_p <- z;  c_z = kappa + T y + E target;  z^0 = y, touched rows q^0 = o_t + a + U_t y;
//                    K times: coef_k from the OLD touched rows (asb_cproj_em_launch, asb_rforce_coef_launch: unchanged),
//                    z <- c_z + sum_k Gz_k coef_k,  q <- o_t + U_t z on the touched rows (k_gsub_expand on the gathered basis)
// State: Z, Z_prev, C_z (3, rq, ld) coordinate-major, frames contiguous, rq = r rounded up to 16 (rows past r zero), ld = n_sel
// rounded up to 64; Qc (3 n_t, ld) in the layout the projection kernels read (CpWorld).
//
//   k_zr_affine      Out = base + sum_seg M_seg X_seg: v_mfma_f64_16x16x4_f64 with A = M (rows x k) and B = X (k x frames).  M is
//                    stored k-major, (3, k, rq): the 16 lanes of an A load read 16 consecutive doubles, as those of a B load do.
//                    A wave owns 16 rows x 16 frames, a block of 4 waves 16 rows x 64 frames; the segments are ONE chain of
//                    MFMAs in slot order, k ascending inside each, from a zero accumulator; then fl(base + acc).  Nothing is
//                    split between blocks, nothing is atomic and no load or store carries a bounds predicate: every operand is
//                    padded (rows to rq, k to a multiple of 4, frames to 64) with zeros.  base: C_z (row stride ld, column
//                    stride 1) or kappa broadcast (1, 0).  An entry does not depend on the chunk, the tile or its neighbours.
//   element-wise     k_zr_carry, k_zr_targets, k_zr_in / k_zr_out (the public (F', r, 3) <-> (3, rq, ld)) and the set-up's fills.
//   k_gsub_expand_diff   a record of a roll-out judged without expanding it: q~ = o + U z formed tile by tile as k_gsub_expand forms it
//                    and compared in registers with a full (F', N, 3) tensor read once (asb_gsub_expand_diff, described at the kernel).
// asb_zroll_steps enqueues every step in stream order and drains ONCE at the end; no host read between steps.
#include "asb_common.h"

#include <algorithm>
#include <cmath>
#include <vector>

typedef double zr_d4 __attribute__((ext_vector_type(4)));

#define ZR_MAX_SLOTS 8
#define ZR_MAX_SEG 8

struct ZrSeg {
    const double *Mt, *X;       // (3, kM, rq) and (3, kX, ldx): kX <= kM rows of Mt are contracted
    int kM, kX;
    long long ldx;
};
struct ZrSegs {
    ZrSeg s[ZR_MAX_SEG];
    int n;
};

struct ZrSlot {
    CpSetup cp;
    long long n_cols = 0;
    double smin = 1.0, smax = 1.0;
    int bank = 0;
};

struct asb_zr {
    bool begun = false, pins = false;
    long long n = 0, n_sel = 0, ld = 0, nt = 0, ntp = 0, r = 0, rq = 0, rp = 0, gen = 0;
    int f0 = 0, fj = 1;
    long long pin_row0 = 0, step = 0, P = 0, Pp = 0;
    double *Z = nullptr, *Zp = nullptr, *Cz = nullptr, *Qc = nullptr;          // 3 x (3, rq, ld); (3 nt, ld)
    double *Tt = nullptr, *kap = nullptr, *Et = nullptr, *tgt = nullptr;       // (3, rq, rq) T^T; (3, rq); (3, Pp, rq) E^T; (3, Pp, ld)
    double *Utt = nullptr, *ot = nullptr, *ota = nullptr, *diag = nullptr;     // (3, rp, ntp); (nt, 3) o_t and o_t + a; (n)
    int* tv = nullptr;
    // the context's force table bound to this roll-out (asb_zroll_forces): Phi^T (3, fTn, rq) k-major like E^T, the touched rows of
    // fa (fTn, 3 nt), and the base of a step's affine product Cb = kappa + Phi[:, rho(c)] (3, rq, ld); fT 0: a constant force
    bool forces = false;
    long long f_row0 = 0, fT = 0, fTn = 0;
    double *Phit = nullptr, *fat = nullptr, *Cb = nullptr;
    int n_slots = 0;
    ZrSlot slot[ZR_MAX_SLOTS];
};

void asb_zroll_free(asb_ctx* ctx) {               // (the buffers went with the context's registered allocations)
    delete ctx->zr;
    ctx->zr = nullptr;
}

// ---------------------------------------------------------------- the affine product
// grid (frame tiles of 64 of the chunk, rq / 16, 3)
__global__ __launch_bounds__(256) void k_zr_affine(const ZrSegs segs, int rq, const double* __restrict__ base, long long brs, long long bcs,
                                                   double* __restrict__ Out, long long ld, long long c0) {
    const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int d = blockIdx.z, j0 = (int)blockIdx.y * 16;
    const long long fx = (long long)blockIdx.x * 64 + wave * 16 + i;          // the column inside the chunk
    zr_d4 acc = zr_d4{0.0, 0.0, 0.0, 0.0};
    for (int sg = 0; sg < segs.n; ++sg) {
        const int kX = segs.s[sg].kX;
        const long long ldx = segs.s[sg].ldx;
        const double* pa = segs.s[sg].Mt + ((long long)d * segs.s[sg].kM + g) * rq + j0 + i;     // A: row j0 + i, k = k0 + g
        const double* pb = segs.s[sg].X + ((long long)d * kX + g) * ldx + fx;                    // B: k = k0 + g, frame fx
        for (int k0 = 0; k0 < kX; k0 += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[(long long)k0 * rq], pb[k0 * ldx], acc, 0, 0, 0);
    }
    // accumulator q of lane (i, g): row g + 4 q of the 16, frame i of the wave's 16
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long long row = (long long)d * rq + j0 + g + 4 * q, col = c0 + fx;
        Out[row * ld + col] = base[row * brs + col * bcs] + acc[q];
    }
}

static void zr_affine_launch(asb_ctx* ctx, const ZrSegs& segs, int rq, const double* base, bool bcast, double* Out, long long ld, long long c0,
                             long long cn) {
    hipLaunchKernelGGL(k_zr_affine, dim3((unsigned)((cn + 63) / 64), (unsigned)(rq / 16), 3), dim3(256), 0, ctx->stream, segs, rq, base,
                       bcast ? 1LL : ld, bcast ? 0LL : 1LL, Out, ld, c0);
}

// ---------------------------------------------------------------- the element-wise kernels
// y = fl(2 z - z_p), z_p <- z, z <- y (2 z is exact: one rounding)
__global__ __launch_bounds__(256) void k_zr_carry(double* __restrict__ Z, double* __restrict__ Zp, long long len) {
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < len; e += (long long)gridDim.x * 256) {
        const double z = Z[e];
        Z[e] = 2.0 * z - Zp[e];
        Zp[e] = z;
    }
}

struct ZrPins {
    const double *p0, *shift;   // shift NULL: fixed pins
    int P, per_pin;
};
// grid (ld / 64, Pp): tgt[d][i][c] = fl(p0[i][d] + shift[row_base + c fj]) for i < P, c < n_sel; 0 elsewhere
__global__ __launch_bounds__(64) void k_zr_targets(ZrPins p, long long row_base, int fj, int n_sel, int Pp, long long ld, double* __restrict__ tgt) {
    const int i = blockIdx.y;
    const long long c = (long long)blockIdx.x * 64 + threadIdx.x;
    const bool on = i < p.P && c < n_sel;
    const long long row = row_base + c * fj;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        double t = 0.0;
        if (on) {
            t = p.p0[3 * i + d];
            if (p.shift) t = t + p.shift[(p.per_pin ? row * p.P + i : row) * 3 + d];
        }
        tgt[((long long)d * Pp + i) * ld + c] = t;
    }
}

// grid (ld / 64, rq, 3): (F, r, 3) -> (3, rq, ld), zero padding;  and back (only j < r, f < F are written)
__global__ __launch_bounds__(64) void k_zr_in(const double* __restrict__ in, int F, int r, int rq, long long ld, double* __restrict__ Z) {
    const int j = blockIdx.y, d = blockIdx.z;
    const long long f = (long long)blockIdx.x * 64 + threadIdx.x;
    Z[((long long)d * rq + j) * ld + f] = (j < r && f < F) ? in[(f * r + j) * 3 + d] : 0.0;
}
__global__ __launch_bounds__(64) void k_zr_out(const double* __restrict__ Z, int F, int r, int rq, long long ld, double* __restrict__ out) {
    const int j = blockIdx.y, d = blockIdx.z;
    const long long f = (long long)blockIdx.x * 64 + threadIdx.x;
    if (j < r && f < F) out[(f * r + j) * 3 + d] = Z[((long long)d * rq + j) * ld + f];
}

// grid (blocks of 64 over rq, rows_out, 3): Out (3, rows_out, rq): Out[d][k][j] = Y[d][j][col0 + k] for k < valid, else 0 (Y (3, rq, ldy))
__global__ __launch_bounds__(64) void k_zr_tr(const double* __restrict__ Y, long long ldy, int col0, int valid, int rows_out, int rq,
                                              double* __restrict__ Out) {
    const int j = (int)blockIdx.x * 64 + threadIdx.x, k = blockIdx.y, d = blockIdx.z;
    if (j >= rq) return;
    Out[((long long)d * rows_out + k) * rq + j] = k < valid ? Y[((long long)d * rq + j) * ldy + col0 + k] : 0.0;
}

// grid (rows, blocks of 64 over ntp), one wave: column tv[t] of src (rows x Np) -> column t of dst (rows x ntp), 0 for t >= nt
__global__ __launch_bounds__(64) void k_zr_gather_cols(const double* __restrict__ src, long long Np, const int* __restrict__ tv, int nt, int ntp,
                                                       double* __restrict__ dst) {
    const long long r = blockIdx.x;
    const int t = (int)blockIdx.y * 64 + threadIdx.x;
    if (t < ntp) dst[r * ntp + t] = t < nt ? src[r * Np + tv[t]] : 0.0;
}
// blocks of 256 over 3 nt: o_t and fl(o_t + a)
__global__ __launch_bounds__(256) void k_zr_gather_o(const double* __restrict__ o, const int* __restrict__ tv, int nt, double a0, double a1, double a2,
                                                     double* __restrict__ ot, double* __restrict__ ota) {
    const int e = (int)blockIdx.x * 256 + threadIdx.x;
    if (e >= 3 * nt) return;
    const int d = e % 3;
    const double x = o[3LL * tv[e / 3] + d];
    ot[e] = x;
    ota[e] = x + (d == 0 ? a0 : (d == 1 ? a1 : a2));
}

// grid (rows / 4, ld / 64): wave = one row 3 v + d x 64 columns of the work matrix R (row length ld):
// R = x_{max(f - back, 0)} - o for the frames f = f0 + c fj, c < n_sel; 0 for the columns past n_sel
__global__ __launch_bounds__(256) void k_zr_frames(CpWorld w, int f0, int fj, int n_sel, long long n_verts, int back, const double* __restrict__ o,
                                                   double* __restrict__ R, long long ld) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long c = (long long)blockIdx.y * 64 + lane;
    if (r >= 3 * n_verts) return;
    double val = 0.0;
    if (c < n_sel) {
        const int v = (int)(r / 3), d = (int)(r % 3);
        long long f = (long long)f0 + c * fj - back;
        f = f > 0 ? f : 0;
        double x[3];
        cp_pos(w, f, v, x);
        val = (d == 0 ? x[0] : (d == 1 ? x[1] : x[2])) - o[r];
    }
    R[r * ld + c] = val;
}
// the same grid: R (filled by k_pd_transpose, columns < F) -= o; columns past F: 0
__global__ __launch_bounds__(256) void k_zr_sub_o(double* __restrict__ R, long long ld, int F, long long n_verts, const double* __restrict__ o) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long c = (long long)blockIdx.y * 64 + lane;
    if (r >= 3 * n_verts) return;
    R[r * ld + c] = c < F ? R[r * ld + c] - o[r] : 0.0;
}

// the same grid: the columns of the set-up's reduce.  Column j < r: D U_d e_j; column r: D (o + a) - A o; the others 0
__global__ __launch_bounds__(256) void k_zr_cols(const double* __restrict__ Un, long long Np, int r, int rq, const double* __restrict__ diag,
                                                 const double* __restrict__ o, const double* __restrict__ Ao, double a0, double a1, double a2,
                                                 long long n_verts, double* __restrict__ R, long long ld) {
    const int lane = threadIdx.x & 63;
    const long long e = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long c = (long long)blockIdx.y * 64 + lane;
    if (e >= 3 * n_verts) return;
    const long long v = e / 3;
    const int d = (int)(e % 3);
    double val = 0.0;
    if (c < r) val = diag[v] * Un[((long long)d * Np + v) * rq + c];
    else if (c == r) val = diag[v] * (o[e] + (d == 0 ? a0 : (d == 1 ? a1 : a2))) - Ao[e];
    R[e * ld + c] = val;
}
// blocks of 256 over 3 P: column i of the (zeroed) work matrix gets w_i at row 3 v_i + d
__global__ __launch_bounds__(256) void k_zr_pin_cols(const int* __restrict__ pv, const double* __restrict__ wi, int P, double* __restrict__ R,
                                                     long long ld) {
    const int e = (int)blockIdx.x * 256 + threadIdx.x;
    if (e >= 3 * P) return;
    const int i = e / 3, d = e % 3;
    R[(3LL * pv[i] + d) * ld + i] = wi[i];
}

// ---- external forces (asb_zroll_forces).  With D fa = force up to the host's rounding, Phi_d = W_d (D o fa_d) (r x rows) joins c_z:
// c_z = kappa + T y + E target + Phi[:, rho(c)], and the touched rows of the first iterate become fl(fl(o_t + a + U_t y) + fa[rho(c)]).
// grid (rows / 4, ldT / 64), as k_zr_cols: column c < Tn of the work matrix is D fa[c] (row 3 v + d), the others 0
__global__ __launch_bounds__(256) void k_zr_force_cols(const double* __restrict__ fa, int Tn, const double* __restrict__ diag, long long n_verts,
                                                       double* __restrict__ R, long long ld) {
    const int lane = threadIdx.x & 63;
    const long long e = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long c = (long long)blockIdx.y * 64 + lane;
    if (e >= 3 * n_verts) return;
    R[e * ld + c] = c < Tn ? diag[e / 3] * fa[c * 3 * n_verts + e] : 0.0;
}
// grid (blocks of 256 over 3 nt, Tn): fat[row][3 t + d] = fa[row][3 tv[t] + d]
__global__ __launch_bounds__(256) void k_zr_force_gather(const double* __restrict__ fa, long long n_verts, const int* __restrict__ tv, int nt,
                                                         double* __restrict__ fat) {
    const int e = (int)blockIdx.x * 256 + threadIdx.x;
    const long long row = blockIdx.y;
    if (e >= 3 * nt) return;
    fat[row * 3 * nt + e] = fa[row * 3 * n_verts + 3LL * tv[e / 3] + e % 3];
}
// grid (ld / 64, rq, 3): Cb[d][j][c] = fl(kappa[d][j] + Phi^T[d][rho(c)][j]), rho(c) = row_base + c fj, for c < n_sel; kappa elsewhere
__global__ __launch_bounds__(64) void k_zr_force_base(const double* __restrict__ kap, const double* __restrict__ Phit, long long Tn, int rq,
                                                      long long row_base, int fj, int n_sel, long long ld, double* __restrict__ Cb) {
    const int j = blockIdx.y, d = blockIdx.z;
    const long long c = (long long)blockIdx.x * 64 + threadIdx.x;
    double v = kap[(long long)d * rq + j];
    if (c < n_sel) v = v + Phit[((long long)d * Tn + row_base + c * fj) * rq + j];
    Cb[((long long)d * rq + j) * ld + c] = v;
}
// grid (3 nt / 4, ld / 64): wave = one touched row 3 t + d x 64 frames: Qc = fl(Qc + fat[rho(c)][3 t + d]) for c < n_sel
__global__ __launch_bounds__(256) void k_zr_force_touched(const double* __restrict__ fat, long long nt3, long long row_base, int fj, int n_sel,
                                                          long long ld, double* __restrict__ Qc) {
    const long long e = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long c = (long long)blockIdx.y * 64 + (threadIdx.x & 63);
    if (e >= nt3 || c >= n_sel) return;
    Qc[e * ld + c] = Qc[e * ld + c] + fat[(row_base + c * fj) * nt3 + e];
}

static void zr_tr_launch(asb_ctx* ctx, const double* Y, long long ldy, int col0, int valid, int rows_out, int rq, double* Out) {
    hipLaunchKernelGGL(k_zr_tr, dim3((unsigned)((rq + 63) / 64), (unsigned)rows_out, 3), dim3(64), 0, ctx->stream, Y, ldy, col0, valid, rows_out, rq, Out);
}

static int zr_view(asb_ctx* ctx, const char* who, GsubView* g) {
    if (!asb_gsub_view(ctx, g)) ASB_FAIL(ctx, ASB_ERR_ARG, "%s: no position subspace on the device (asb_gsub_setup)", who);
    return ASB_OK;
}

// ---------------------------------------------------------------- the operator of the current bank
extern "C" int asb_zroll_operator(asb_ctx* ctx) {
    if (!ctx) return ASB_ERR_ARG;
    asb_ctx::RfBank& b = asb_rf_cur(ctx);
    b.zok = 0;
    GsubView g;
    int rc;
    if ((rc = zr_view(ctx, "asb_zroll_operator", &g))) return rc;
    if (b.mp < 1 || !b.M) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_operator: no operator S^T V on the device (asb_rforce_operator)");
    if (b.n != g.n || g.n != ctx->n_loc)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_operator: the subspace has %lld rows, S^T V %lld, the tensor %lld vertices", g.n, (long long)b.n,
                 (long long)ctx->n_loc);
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    if ((rc = asb_alloc(ctx, &b.Gz, (size_t)3 * b.mpp * g.rq))) return rc;
    long long ldm = 0;
    double* Y = nullptr;
    if ((rc = asb_gsub_rows_in(ctx, b.M, 3 * b.mpp, b.Np, &ldm, &Y))) return rc;
    zr_tr_launch(ctx, Y, ldm, 0, (int)b.mpp, (int)b.mpp, (int)g.rq, b.Gz);
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    b.zok = 1;
    return ASB_OK;
}

// ---------------------------------------------------------------- coordinates and expansion
// R (3 Np, ld) <- the selected frames minus o (pos_dev: a caller's frame-major tensor of F frames instead), shifted back by `back`
static void zr_fill_frames(asb_ctx* ctx, const GsubView& g, const CpWorld* w, int f0, int fj, long long F, int back, const double* pos_dev, double* R,
                           long long ld) {
    const dim3 grid((unsigned)((3 * g.n + 3) / 4), (unsigned)(ld / 64));
    if (pos_dev) {
        asb_pd_transpose_launch(ctx, pos_dev, (int)F, 3 * g.n, R, ld);
        hipLaunchKernelGGL(k_zr_sub_o, grid, dim3(256), 0, ctx->stream, R, ld, (int)F, g.n, g.o);
    } else {
        hipLaunchKernelGGL(k_zr_frames, grid, dim3(256), 0, ctx->stream, *w, f0, fj, (int)F, g.n, back, g.o, R, ld);
    }
}

extern "C" int asb_gsub_coordinates(asb_ctx* ctx, int which, int64_t f0, int64_t f1, int64_t fj, const double* inv_massL, int add_mean, double psf,
                                    const double* pos_dev, int64_t n_frames, double* out_dev) {
    if (!ctx || !out_dev) return ASB_ERR_ARG;
    if (pos_dev && (n_frames < 1 || (n_frames + 63) / 64 > 65535)) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_gsub_coordinates: %lld frames", (long long)n_frames);
    GsubView g;
    int rc;
    if ((rc = zr_view(ctx, "asb_gsub_coordinates", &g))) return rc;
    CpWorld w = {};
    int64_t n_sel = n_frames;
    if (!pos_dev) {
        if (fj >= 1 && f1 > f0 && ((f1 - f0 + fj - 1) / fj + 63) / 64 > 65535)
            ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_gsub_coordinates: %lld frames in one call (at most %d)", (long long)((f1 - f0 + fj - 1) / fj), 65535 * 64);
        if ((rc = asb_world_frames(ctx, "asb_gsub_coordinates", which, f0, f1, fj, add_mean, psf, &w, &n_sel))) return rc;
    }
    if (ctx->n_loc != g.n) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_gsub_coordinates: the subspace has %lld vertices, the tensor %lld", g.n, (long long)ctx->n_loc);
    if (!pos_dev && (rc = asb_cproj_invm(ctx, inv_massL, &w))) return rc;
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    const long long ld = (n_sel + 63) / 64 * 64;
    double *R = nullptr, *Y = nullptr;
    if ((rc = asb_gsub_work(ctx, ld, &R, &Y))) return rc;
    zr_fill_frames(ctx, g, &w, (int)f0, (int)fj, n_sel, 0, pos_dev, R, ld);
    asb_gsub_reduce_launch(ctx, 1, ld, Y);
    hipLaunchKernelGGL(k_zr_out, dim3((unsigned)(ld / 64), (unsigned)g.rq, 3), dim3(64), 0, ctx->stream, Y, (int)n_sel, (int)g.r, (int)g.rq, ld, out_dev);
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));          // the caller owns both tensors and may use them on any stream
    return ASB_OK;
}

extern "C" int asb_gsub_expand(asb_ctx* ctx, const double* z_dev, int64_t n_frames, double* out_dev) {
    if (!ctx || n_frames < 1 || !z_dev || !out_dev) return ASB_ERR_ARG;
    if ((n_frames + 63) / 64 > 65535) ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_gsub_expand: %lld frames in one call (at most %d)", (long long)n_frames, 65535 * 64);
    GsubView g;
    int rc;
    if ((rc = zr_view(ctx, "asb_gsub_expand", &g))) return rc;
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    const long long ld = (n_frames + 63) / 64 * 64;
    asb_tmp<double> Z, Qv;
    if ((rc = Z.alloc(ctx, (size_t)3 * g.rq * ld)) || (rc = Qv.alloc(ctx, (size_t)3 * g.n * ld))) return rc;
    hipLaunchKernelGGL(k_zr_in, dim3((unsigned)(ld / 64), (unsigned)g.rq, 3), dim3(64), 0, ctx->stream, z_dev, (int)n_frames, (int)g.r, (int)g.rq, ld, Z.get());
    asb_gsub_expand_launch(ctx, g.Ut, g.Np, Z.get(), ld, g.o, Qv.get(), n_frames, g.n, out_dev);
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ASB_OK;
}

// ---------------------------------------------------------------- the expansion compared where it is formed (asb_gsub_expand_diff)
// The metrics of asb_force_diff(a, o + U z) without o + U z in memory.  A block of 4 waves owns 64 frames and the vertex tiles
// [blockIdx.y tpg, + tpg) of 32, walked in ascending order; per tile
//   q~      the MFMA chain of k_gsub_expand (asb_gsub.hip) operand for operand: A = U^T (vertices x k), B = Z (k x frames), k ascending
//           from a zero accumulator, then fl(o + acc) -- the bits of asb_gsub_expand, whatever the tile, the width or the neighbours
//   a       the tile's 64 runs of 96 doubles (32 vertices x 3) are read once, coalesced -- half a wave reads 32 consecutive doubles
//           of a frame's run, a thread 3 x 8 of them -- into registers BEFORE the chain of the tile, which hides them, and go through
//           LDS rows of 97 doubles into the accumulator layout (the FM branch of k_gsub_expand, run backwards): lane (i, g) of
//           wave w reads frame 16 w + i, vertices g + 4 q and 16 + g + 4 q
//   record  the arithmetic of k_force_diff per entry, in a lane ascending in the vertex over all its tiles; the 4 lanes of a frame
//           are combined g = 0, 1, 2, 3 and lane g = 0 writes the record of (group, frame) -- no atomics
// Vertices >= n and frames >= F contribute nothing (their records stay 0 / -inf) and no address is formed for them.
// k_gsub_diff_frames then adds a frame's groups in ascending order into the FD_REC records k_force_diff_final combines.  The
// split into groups depends on N alone: a frame's record does not depend on the number of frames or on the frames beside it.
#define ZD_TN 32            // vertices per tile and frames per block: those of k_gsub_expand
#define ZD_TF 64
#define ZD_GROUPS 256       // at most this many blocks share the vertices of a frame tile

// grid (ld / 64, groups); Ut (3, rp, Np); Z (3, rq, ld); o (n, 3); a (F, n, 3); part (groups, ld, FD_REC)
__global__ __launch_bounds__(256) void k_gsub_expand_diff(const double* __restrict__ Ut, long long Np, int rp, const double* __restrict__ Z, int rq,
                                                          long long ld, const double* __restrict__ o, const double* __restrict__ a, int F, int n,
                                                          int tpg, double* __restrict__ part) {
    constexpr int RUN = ZD_TN * 3, ROW = RUN + 1, NJ = ZD_TF / 8;
    __shared__ double stage[ZD_TF * ROW];
    const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t0 = (int)blockIdx.x * ZD_TF;
    const int nf = F - t0 < ZD_TF ? F - t0 : ZD_TF;
    const int fl = wave * 16 + i;
    const bool fok = fl < nf;
    const int tiles = (int)(Np / ZD_TN), tb = (int)blockIdx.y * tpg, te = tb + tpg < tiles ? tb + tpg : tiles;
    const int col = threadIdx.x & 31, fr0 = threadIdx.x >> 5;          // a: doubles col, col + 32, col + 64 of the runs of frames fr0 + 8 j
    double x[FD_REC] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -INFINITY};
    const double* pb = Z + t0 + wave * 16 + i;                        // B: k = g, frame i of the wave's 16
    for (int tile = tb; tile < te; ++tile) {
        const int v0 = tile * ZD_TN;                                  // (v0 < n always: Np - n < 32)
        const int run = (n - v0 < ZD_TN ? n - v0 : ZD_TN) * 3;
        double ar[NJ][3];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int fr = fr0 + 8 * j;
            const double* row = a + ((long long)(t0 + fr) * n + v0) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) ar[j][c] = (fr < nf && col + 32 * c < run) ? row[col + 32 * c] : 0.0;
        }
        zr_d4 acc[3][2];
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int y = 0; y < 2; ++y) acc[d][y] = zr_d4{0.0, 0.0, 0.0, 0.0};
        const double* pa = Ut + v0 + i;                               // A: vertex i of 16, k = g
        for (int k0 = 0; k0 < rp; k0 += 4) {
            const int k = k0 + g;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double* ua = pa + ((long long)d * rp + k) * Np;
                const double b = pb[((long long)d * rq + k) * ld];
                acc[d][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(ua[0], b, acc[d][0], 0, 0, 0);
                acc[d][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(ua[16], b, acc[d][1], 0, 0, 0);
            }
        }
        __syncthreads();                                              // the tile before has been read out of the stage
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) stage[(fr0 + 8 * j) * ROW + col + 32 * c] = ar[j][c];
        __syncthreads();
        // accumulator q of lane (i, g): vertex g + 4 q of the 16, frame i of the wave's 16
#pragma unroll
        for (int d = 0; d < 3; ++d) {
#pragma unroll
            for (int y = 0; y < 2; ++y)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int vl = 16 * y + g + 4 * q;
                    if (fok && v0 + vl < n) {
                        const double val = o[3LL * (v0 + vl) + d] + acc[d][y][q];
                        const double av = stage[fl * ROW + vl * 3 + d], e = av - val;
                        x[d] = fma(e, e, x[d]);
                        x[3 + d] = fma(av, av, x[3 + d]);
                        x[6] = fmax(x[6], fabs(e));
                        x[7] = fmax(x[7], av);
                    }
                }
        }
    }
    // the frame's four lanes, g ascending
#pragma unroll
    for (int s = 1; s < 4; ++s) {
        double y[FD_REC];
#pragma unroll
        for (int q = 0; q < FD_REC; ++q) y[q] = __shfl(x[q], i + 16 * s, 64);
        if (g == 0) fd_combine(x, y);
    }
    if (g == 0) {
        double* p = part + ((long long)blockIdx.y * ld + t0 + fl) * FD_REC;
#pragma unroll
        for (int q = 0; q < FD_REC; ++q) p[q] = x[q];
    }
}

// blocks of 256 over the frames: rec[f] = the records of frame f's groups, ascending
__global__ __launch_bounds__(256) void k_gsub_diff_frames(const double* __restrict__ part, long long ld, int groups, int F, double* __restrict__ rec) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    double x[FD_REC] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -INFINITY};
    for (int gi = 0; gi < groups; ++gi) fd_combine(x, part + ((long long)gi * ld + f) * FD_REC);
#pragma unroll
    for (int q = 0; q < FD_REC; ++q) rec[f * FD_REC + q] = x[q];
}

extern "C" int asb_gsub_expand_diff(asb_ctx* ctx, const double* a_dev, const double* z_dev, int64_t n_frames, double* sums_out, double* max_out,
                                    double* norms_out, double* per_frame_out) {
    if (!ctx || n_frames < 1 || !a_dev || !z_dev) return ASB_ERR_ARG;
    if ((n_frames + 63) / 64 > 65535)
        ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_gsub_expand_diff: %lld frames in one call (at most %d)", (long long)n_frames, 65535 * 64);
    GsubView g;
    int rc;
    if ((rc = zr_view(ctx, "asb_gsub_expand_diff", &g))) return rc;
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    const long long ld = (n_frames + 63) / 64 * 64, tiles = g.Np / ZD_TN;
    const long long tpg = (tiles + ZD_GROUPS - 1) / ZD_GROUPS, groups = (tiles + tpg - 1) / tpg;
    asb_tmp<double> Z, part, rec;
    if ((rc = Z.alloc(ctx, (size_t)3 * g.rq * ld)) || (rc = part.alloc(ctx, (size_t)groups * ld * FD_REC)) ||
        (rc = rec.alloc(ctx, (size_t)(n_frames + 1) * FD_REC)))
        return rc;
    hipLaunchKernelGGL(k_zr_in, dim3((unsigned)(ld / 64), (unsigned)g.rq, 3), dim3(64), 0, ctx->stream, z_dev, (int)n_frames, (int)g.r, (int)g.rq, ld, Z.get());
    hipLaunchKernelGGL(k_gsub_expand_diff, dim3((unsigned)(ld / ZD_TF), (unsigned)groups), dim3(256), 0, ctx->stream, g.Ut, g.Np, (int)g.rp, Z.get(),
                       (int)g.rq, ld, g.o, a_dev, (int)n_frames, (int)g.n, (int)tpg, part.get());
    hipLaunchKernelGGL(k_gsub_diff_frames, dim3((unsigned)((n_frames + 255) / 256)), dim3(256), 0, ctx->stream, part.get(), ld, (int)groups,
                       (int)n_frames, rec.get());
    asb_force_diff_final_launch(ctx, rec.get(), (long long)n_frames);
    ASB_CHECK_LAUNCH(ctx);
    return asb_force_diff_outputs(ctx, rec.get(), (long long)n_frames, sums_out, max_out, norms_out, per_frame_out);
}

// ---------------------------------------------------------------- the roll-out
extern "C" int asb_zroll_begin(asb_ctx* ctx, int which, int64_t f0, int64_t f1, int64_t fj, const double* inv_massL, int add_mean, double psf,
                               const double* diag, int mode, const double* acc3, int64_t n_touched, const int64_t* touched, const double* z_dev,
                               const double* zprev_dev) {
    if (!ctx || n_touched < 1 || !diag || !acc3 || !touched) return ASB_ERR_ARG;
    if (ctx->zr) ctx->zr->begun = false, ctx->zr->n_slots = 0, ctx->zr->pins = false, ctx->zr->forces = false;
    if (fj >= 1 && f1 > f0 && ((f1 - f0 + fj - 1) / fj + 63) / 64 > 65535)        // on the count alone, before any tensor is looked at
        ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_zroll_begin: %lld frames in one roll-out (at most %d)", (long long)((f1 - f0 + fj - 1) / fj), 65535 * 64);
    if (mode != 0 && mode != 1) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_begin: mode %d (0: z_prev = z, 1: z_prev from the previous frame)", mode);
    if ((z_dev == nullptr) != (zprev_dev == nullptr)) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_begin: a continuation needs both z and z_prev");
    GsubView g;
    int rc;
    if ((rc = zr_view(ctx, "asb_zroll_begin", &g))) return rc;
    CpWorld w;
    int64_t n_sel;
    if ((rc = asb_world_frames(ctx, "asb_zroll_begin", which, f0, f1, fj, add_mean, psf, &w, &n_sel))) return rc;
    const long long n = ctx->n_loc, nt = n_touched;
    if (g.n != n) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_begin: the subspace has %lld vertices, the tensor %lld", g.n, n);
    if (nt > n) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_begin: %lld touched vertices of %lld", nt, n);
    for (long long t = 0; t < nt; ++t)
        if (touched[t] < 0 || touched[t] >= n || (t > 0 && touched[t] <= touched[t - 1]))
            ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_begin: touched[%lld] = %lld: ascending vertices of 0..%lld", t, (long long)touched[t], n - 1);
    for (long long v = 0; v < n; ++v)
        if (!std::isfinite(diag[v])) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_begin: diag[%lld] is not finite", v);
    if (!std::isfinite(acc3[0]) || !std::isfinite(acc3[1]) || !std::isfinite(acc3[2])) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_begin: acc is not finite");
    if ((rc = asb_cproj_invm(ctx, inv_massL, &w))) return rc;
    if (!ctx->zr) ctx->zr = new asb_zr();
    asb_zr* s = ctx->zr;
    const long long ld = (n_sel + 63) / 64 * 64, ntp = (nt + 31) / 32 * 32, rq = g.rq, rp = g.rp;
    const size_t zl = (size_t)3 * rq * ld;
    if ((rc = asb_alloc(ctx, &s->Z, zl)) || (rc = asb_alloc(ctx, &s->Zp, zl)) || (rc = asb_alloc(ctx, &s->Cz, zl))) return rc;
    if ((rc = asb_alloc(ctx, &s->Qc, (size_t)3 * nt * ld)) || (rc = asb_alloc(ctx, &s->Tt, (size_t)3 * rq * rq))) return rc;
    if ((rc = asb_alloc(ctx, &s->kap, (size_t)3 * rq)) || (rc = asb_alloc(ctx, &s->Utt, (size_t)3 * rp * ntp))) return rc;
    if ((rc = asb_alloc(ctx, &s->ot, (size_t)3 * nt)) || (rc = asb_alloc(ctx, &s->ota, (size_t)3 * nt))) return rc;
    if ((rc = asb_alloc(ctx, &s->tv, (size_t)nt)) || (rc = asb_alloc(ctx, &s->diag, (size_t)n))) return rc;
    std::vector<int> t32((size_t)nt);
    for (long long t = 0; t < nt; ++t) t32[t] = (int)touched[t];
    ASB_HIP(ctx, hipMemcpyAsync(s->tv, t32.data(), (size_t)nt * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemcpyAsync(s->diag, diag, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ASB_HIP(ctx, hipMemsetAsync(s->Qc, 0, (size_t)3 * nt * ld * sizeof(double), ctx->stream));       // the padding columns, once
    hipLaunchKernelGGL(k_zr_gather_cols, dim3((unsigned)(3 * rp), (unsigned)((ntp + 63) / 64)), dim3(64), 0, ctx->stream, g.Ut, g.Np, s->tv, (int)nt,
                       (int)ntp, s->Utt);
    hipLaunchKernelGGL(k_zr_gather_o, dim3((unsigned)((3 * nt + 255) / 256)), dim3(256), 0, ctx->stream, g.o, s->tv, (int)nt, acc3[0], acc3[1], acc3[2],
                       s->ot, s->ota);
    // ---- T and kappa: one reduce on r + 1 columns
    double *R = nullptr, *Y = nullptr;
    const long long lds = (g.r + 1 + 63) / 64 * 64;
    if ((rc = asb_gsub_work(ctx, lds, &R, &Y))) return rc;
    hipLaunchKernelGGL(k_zr_cols, dim3((unsigned)((3 * n + 3) / 4), (unsigned)(lds / 64)), dim3(256), 0, ctx->stream, g.Un, g.Np, (int)g.r, (int)rq,
                       s->diag, g.o, g.Ao, acc3[0], acc3[1], acc3[2], n, R, lds);
    asb_gsub_reduce_launch(ctx, 0, lds, Y);
    zr_tr_launch(ctx, Y, lds, 0, (int)g.r, (int)rq, (int)rq, s->Tt);
    zr_tr_launch(ctx, Y, lds, (int)g.r, 1, 1, (int)rq, s->kap);
    ASB_CHECK_LAUNCH(ctx);
    // ---- the state
    const dim3 gz((unsigned)(ld / 64), (unsigned)rq, 3);
    if (z_dev) {
        hipLaunchKernelGGL(k_zr_in, gz, dim3(64), 0, ctx->stream, z_dev, (int)n_sel, (int)g.r, (int)rq, ld, s->Z);
        hipLaunchKernelGGL(k_zr_in, gz, dim3(64), 0, ctx->stream, zprev_dev, (int)n_sel, (int)g.r, (int)rq, ld, s->Zp);
    } else {
        if ((rc = asb_gsub_work(ctx, ld, &R, &Y))) return rc;
        zr_fill_frames(ctx, g, &w, (int)f0, (int)fj, n_sel, 0, nullptr, R, ld);
        asb_gsub_reduce_launch(ctx, 1, ld, s->Z);
        if (mode == 1) {
            zr_fill_frames(ctx, g, &w, (int)f0, (int)fj, n_sel, 1, nullptr, R, ld);
            asb_gsub_reduce_launch(ctx, 1, ld, s->Zp);
        } else {
            ASB_HIP(ctx, hipMemcpyAsync(s->Zp, s->Z, zl * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        }
    }
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));          // the host arrays and the caller's state may go
    s->n = n, s->n_sel = n_sel, s->ld = ld, s->nt = nt, s->ntp = ntp, s->r = g.r, s->rq = rq, s->rp = rp, s->gen = g.gen;
    s->f0 = (int)f0, s->fj = (int)fj, s->step = 0, s->pin_row0 = 0, s->P = s->Pp = 0;
    s->begun = true;
    return ASB_OK;
}

extern "C" int asb_zroll_slot(asb_ctx* ctx, double sigma_min, double sigma_max) {
    if (!ctx) return ASB_ERR_ARG;
    asb_zr* s = ctx->zr;
    if (!s || !s->begun) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_slot: no roll-out begun (asb_zroll_begin)");
    if (s->n_slots >= ZR_MAX_SLOTS) ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_zroll_slot: more than %d kinds", ZR_MAX_SLOTS);
    if (ctx->cp.kind < 0 || ctx->cp.verts != s->n || ctx->n_loc != s->n)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_slot: no element set-up for the resident tensor (asb_cproj_setup)");
    if (!(sigma_min <= sigma_max)) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_slot: sigma_min %g > sigma_max %g", sigma_min, sigma_max);
    const long long n_cols = asb_cproj_rows(ctx->cp.kind, ctx->cp.n);
    const asb_ctx::RfBank& b = asb_rf_cur(ctx);
    for (int k = 0; k < s->n_slots; ++k)
        if (s->slot[k].bank == ctx->rf_cur)
            ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_slot: a second reduced kind on bank %d (asb_rforce_bank before the operator)", ctx->rf_cur);
    if (b.mp < 1 || b.r < 1 || b.n != s->n)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_slot: no operator or solver for the tensor on the device (asb_rforce_operator, asb_rforce_solver)");
    if (b.pt_max >= n_cols)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_slot: an interpolation point names row %lld, the sampled elements have %lld", (long long)b.pt_max, n_cols);
    if (ctx->cp.vmax >= s->nt)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_slot: the element set-up names vertex %lld, the iterate has %lld rows", (long long)ctx->cp.vmax, s->nt);
    ZrSlot& p = s->slot[s->n_slots];
    asb_cp_move(ctx, ctx->cp, p.cp);
    p.n_cols = n_cols, p.smin = sigma_min, p.smax = sigma_max, p.bank = ctx->rf_cur;
    ++s->n_slots;
    return ASB_OK;
}

extern "C" int asb_zroll_pins(asb_ctx* ctx, int64_t row0) {
    if (!ctx) return ASB_ERR_ARG;
    asb_zr* s = ctx->zr;
    if (!s || !s->begun) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_pins: no roll-out begun (asb_zroll_begin)");
    if (s->pins) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_pins: the roll-out has its pins already");
    if (row0 < 0) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_pins: row0 %lld", (long long)row0);
    const asb_ctx::Pins& h = ctx->pins;
    if (h.P < 1) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_pins: no pins on the device (asb_pins_set)");
    if (h.n != s->n || ctx->n_loc != s->n)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_pins: the pins were checked against %lld vertices, the roll-out has %lld", (long long)h.n, s->n);
    if (h.P + 3 > 65535) ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_zroll_pins: %lld pins (at most 65532: they sit on one grid dimension)", (long long)h.P);
    GsubView g;
    int rc;
    if ((rc = zr_view(ctx, "asb_zroll_pins", &g))) return rc;
    if (g.gen != s->gen) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_pins: the subspace changed since asb_zroll_begin");
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    const long long P = h.P, Pp = (P + 3) / 4 * 4, ldp = (P + 63) / 64 * 64;
    if ((rc = asb_alloc(ctx, &s->Et, (size_t)3 * Pp * s->rq)) || (rc = asb_alloc(ctx, &s->tgt, (size_t)3 * Pp * s->ld))) return rc;
    double *R = nullptr, *Y = nullptr;
    if ((rc = asb_gsub_work(ctx, ldp, &R, &Y))) return rc;
    ASB_HIP(ctx, hipMemsetAsync(R, 0, (size_t)3 * g.Np * ldp * sizeof(double), ctx->stream));
    hipLaunchKernelGGL(k_zr_pin_cols, dim3((unsigned)((3 * P + 255) / 256)), dim3(256), 0, ctx->stream, h.v, h.wi, (int)P, R, ldp);
    asb_gsub_reduce_launch(ctx, 0, ldp, Y);
    zr_tr_launch(ctx, Y, ldp, 0, (int)P, (int)Pp, (int)s->rq, s->Et);
    ASB_CHECK_LAUNCH(ctx);
    s->pin_row0 = row0, s->P = P, s->Pp = Pp, s->pins = true;
    return ASB_OK;
}

// Binds the force table of asb_ext_set to the roll-out.  ALL rows of the table are prepared here, once (Tn = T_s, or 1 for a constant
// force): which rows a later asb_zroll_steps(n_steps) reads is not known yet, and a continuation reads further ones.  Phi = W (D fa^T)
// through the reduce of asb_gsub.hip, the table's rows its columns: one chain over N per entry, ascending, never split.
extern "C" int asb_zroll_forces(asb_ctx* ctx, int64_t row0) {
    if (!ctx) return ASB_ERR_ARG;
    asb_zr* s = ctx->zr;
    if (!s || !s->begun) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_forces: no roll-out begun (asb_zroll_begin)");
    if (s->forces) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_forces: the roll-out has its forces already");
    if (row0 < 0) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_forces: row0 %lld", (long long)row0);
    const asb_ctx::Ext& h = ctx->ext;
    if (h.n < 1 || !h.force) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_forces: no force table on the device (asb_ext_set)");
    if (h.floor) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_forces: a floor is set: a clamp on vertex coordinates has no form in z");
    if (h.n != s->n || ctx->n_loc != s->n)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_forces: the forces were checked against %lld vertices, the roll-out has %lld", (long long)h.n, s->n);
    const long long Tn = h.T > 0 ? h.T : 1;
    if (Tn > 65535) ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_zroll_forces: %lld rows of the force table (at most 65535: they sit on one grid dimension)", Tn);
    if (h.T > 0 && row0 + s->f0 + (s->n_sel - 1) * s->fj + s->step >= h.T)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_forces: row %lld of the force table is needed, it has %lld", row0 + s->f0 + (s->n_sel - 1) * s->fj + s->step,
                 (long long)h.T);
    GsubView g;
    int rc;
    if ((rc = zr_view(ctx, "asb_zroll_forces", &g))) return rc;
    if (g.gen != s->gen) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_forces: the subspace changed since asb_zroll_begin");
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    const long long ldT = (Tn + 63) / 64 * 64;
    if ((rc = asb_alloc(ctx, &s->Phit, (size_t)3 * Tn * s->rq)) || (rc = asb_alloc(ctx, &s->fat, (size_t)Tn * 3 * s->nt))) return rc;
    if ((rc = asb_alloc(ctx, &s->Cb, (size_t)3 * s->rq * s->ld))) return rc;
    double *R = nullptr, *Y = nullptr;
    if ((rc = asb_gsub_work(ctx, ldT, &R, &Y))) return rc;
    hipLaunchKernelGGL(k_zr_force_cols, dim3((unsigned)((3 * s->n + 3) / 4), (unsigned)(ldT / 64)), dim3(256), 0, ctx->stream, h.fa, (int)Tn, s->diag, s->n,
                       R, ldT);
    asb_gsub_reduce_launch(ctx, 0, ldT, Y);
    zr_tr_launch(ctx, Y, ldT, 0, (int)Tn, (int)Tn, (int)s->rq, s->Phit);
    hipLaunchKernelGGL(k_zr_force_gather, dim3((unsigned)((3 * s->nt + 255) / 256), (unsigned)Tn), dim3(256), 0, ctx->stream, h.fa, s->n, s->tv,
                       (int)s->nt, s->fat);
    ASB_CHECK_LAUNCH(ctx);
    s->f_row0 = row0, s->fT = h.T, s->fTn = Tn, s->forces = true;
    return ASB_OK;
}

extern "C" int asb_zroll_steps(asb_ctx* ctx, int64_t n_steps, int64_t n_iter, int64_t chunk_frames, int64_t record_every, double* records_dev) {
    if (!ctx) return ASB_ERR_ARG;
    asb_zr* s = ctx->zr;
    if (!s || !s->begun || s->n_slots < 1) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_steps: no roll-out begun or no kind registered (asb_zroll_begin, asb_zroll_slot)");
    if (n_steps < 1 || n_steps > (1 << 20)) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_steps: %lld time steps", (long long)n_steps);
    if (n_iter < 1 || n_iter > (1 << 20)) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_steps: %lld iterations", (long long)n_iter);
    if (chunk_frames < 0) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_steps: chunk_frames %lld", (long long)chunk_frames);
    if (record_every < 0 || (record_every > 0 && !records_dev)) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_steps: record_every %lld without a tensor for the records", (long long)record_every);
    GsubView g;
    int rc;
    if ((rc = zr_view(ctx, "asb_zroll_steps", &g))) return rc;
    if (g.gen != s->gen || g.n != s->n || ctx->n_loc != s->n)
        ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_steps: the subspace or the tensor changed since asb_zroll_begin");
    const int ns = s->n_slots;
    asb_ctx::RfBank* bank[ZR_MAX_SLOTS] = {};
    for (int k = 0; k < ns; ++k) {
        bank[k] = &ctx->rf_bank[s->slot[k].bank];
        if (bank[k]->mp < 1 || bank[k]->r < 1 || bank[k]->n != s->n || bank[k]->pt_max >= s->slot[k].n_cols)
            ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_steps: the operator or solver changed since asb_zroll_slot");
        if (!bank[k]->zok || !bank[k]->Gz)
            ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_steps: no operator (U^T A U)^-1 U^T S^T V for the subspace and the basis on the device "
                                       "(asb_zroll_operator after asb_gsub_setup and asb_rforce_operator): a stale one is refused");
    }
    const asb_ctx::Pins& h = ctx->pins;
    if (s->pins) {
        if (h.P != s->P || h.n != s->n) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_steps: the pins changed since asb_zroll_pins");
        const long long last = s->pin_row0 + s->f0 + (s->n_sel - 1) * s->fj + s->step + n_steps - 1;
        if (h.T > 0 && last >= h.T) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_steps: row %lld of the shift is needed, it has %lld", last, (long long)h.T);
    }
    if (s->forces) {
        const asb_ctx::Ext& e = ctx->ext;
        if (!e.force || e.n != s->n || e.T != s->fT) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_steps: the forces changed since asb_zroll_forces");
        const long long last = s->f_row0 + s->f0 + (s->n_sel - 1) * s->fj + s->step + n_steps - 1;
        if (s->fT > 0 && last >= s->fT) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_steps: row %lld of the force table is needed, it has %lld", last, s->fT);
    }
    const long long n_sel = s->n_sel, ld = s->ld, rq = s->rq;
    long long cw = 0, cols_max = 0;
    for (int k = 0; k < ns; ++k) {
        const long long w = asb_rforce_chunk_width(bank[k]->r, s->slot[k].n_cols, n_sel);
        cw = k == 0 ? w : std::min(cw, w);
        cols_max = std::max(cols_max, s->slot[k].n_cols);
    }
    if (chunk_frames > 0) cw = std::min<long long>(cw, (chunk_frames + 63) / 64 * 64);
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    if ((rc = asb_alloc(ctx, &ctx->cf_scratch, (size_t)3 * cols_max * cw))) return rc;
    ZrSegs upd = {}, adv = {};
    upd.n = ns;
    for (int k = 0; k < ns; ++k) {
        const int rpp = ((int)bank[k]->r + 3) / 4 * 4;
        if ((rc = asb_alloc(ctx, &bank[k]->coef, (size_t)3 * rpp * cw))) return rc;
        upd.s[k] = ZrSeg{bank[k]->Gz, bank[k]->coef, (int)bank[k]->mpp, rpp, cw};
    }
    adv.n = s->pins ? 2 : 1;
    adv.s[0] = ZrSeg{s->Tt, s->Z, (int)rq, (int)rq, ld};
    if (s->pins) adv.s[1] = ZrSeg{s->Et, s->tgt, (int)s->Pp, (int)s->Pp, ld};
    const ZrPins zp = {h.p0, h.T > 0 ? h.shift : nullptr, (int)h.P, h.per_pin};
    const CpWorld wq = {s->Qc, ld, nullptr, nullptr, 1.0};
    const long long zl = 3 * rq * ld;
    const unsigned g_carry = (unsigned)std::min<long long>((zl + 255) / 256, 1 << 16);
    const size_t rec_len = (size_t)n_sel * s->r * 3;
    long long n_rec = 0;
    for (int64_t t = 1; t <= n_steps; ++t) {
        hipLaunchKernelGGL(k_zr_carry, dim3(g_carry), dim3(256), 0, ctx->stream, s->Z, s->Zp, zl);
        if (s->pins)
            hipLaunchKernelGGL(k_zr_targets, dim3((unsigned)(ld / 64), (unsigned)s->Pp), dim3(64), 0, ctx->stream, zp, s->pin_row0 + s->f0 + s->step, s->fj,
                               (int)n_sel, (int)s->Pp, ld, s->tgt);
        if (s->forces) {                            // two launches more: the base with Phi's column of every frame, and fa on the touched rows
            const long long fr = s->fT > 0 ? s->f_row0 + s->f0 + s->step : 0;
            const int ffj = s->fT > 0 ? s->fj : 0;
            hipLaunchKernelGGL(k_zr_force_base, dim3((unsigned)(ld / 64), (unsigned)rq, 3), dim3(64), 0, ctx->stream, s->kap, s->Phit, s->fTn, (int)rq, fr,
                               ffj, (int)n_sel, ld, s->Cb);
            zr_affine_launch(ctx, adv, (int)rq, s->Cb, false, s->Cz, ld, 0, ld);
            asb_gsub_expand_launch(ctx, s->Utt, s->ntp, s->Z, ld, s->ota, s->Qc, n_sel, s->nt, nullptr);
            hipLaunchKernelGGL(k_zr_force_touched, dim3((unsigned)((3 * s->nt + 3) / 4), (unsigned)(ld / 64)), dim3(256), 0, ctx->stream, s->fat, 3 * s->nt,
                               fr, ffj, (int)n_sel, ld, s->Qc);
        } else {
            zr_affine_launch(ctx, adv, (int)rq, s->kap, true, s->Cz, ld, 0, ld);
            asb_gsub_expand_launch(ctx, s->Utt, s->ntp, s->Z, ld, s->ota, s->Qc, n_sel, s->nt, nullptr);
        }
        for (int64_t it = 0; it < n_iter; ++it) {
            for (long long c0 = 0; c0 < n_sel; c0 += cw) {
                const int cn = (int)(c0 + cw < n_sel ? cw : n_sel - c0);
                // ALL coefficients from the old touched rows, then one launch writes z: a Jacobi update over the kinds
                for (int k = 0; k < ns; ++k) {
                    const ZrSlot& p = s->slot[k];
                    asb_cproj_em_launch(ctx, p.cp, wq, 0, 1, (int)c0, cn, (int)cw, p.smin, p.smax, ctx->cf_scratch);
                    asb_rforce_coef_launch(ctx, *bank[k], ctx->cf_scratch, (int)cw, cn);
                }
                zr_affine_launch(ctx, upd, (int)rq, s->Cz, false, s->Z, ld, c0, cn);
            }
            if (it + 1 < n_iter)                    // (the next step's first iterate comes from y: the last expansion is not needed)
                asb_gsub_expand_launch(ctx, s->Utt, s->ntp, s->Z, ld, s->ot, s->Qc, n_sel, s->nt, nullptr);
        }
        ++s->step;
        if (record_every > 0 && t % record_every == 0)
            hipLaunchKernelGGL(k_zr_out, dim3((unsigned)(ld / 64), (unsigned)rq, 3), dim3(64), 0, ctx->stream, s->Z, (int)n_sel, (int)s->r, (int)rq, ld,
                               records_dev + (size_t)(n_rec++) * rec_len);
    }
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));          // the one drain: the caller owns the records and may read them on any stream
    return ASB_OK;
}

extern "C" int asb_zroll_state(asb_ctx* ctx, double* z_dev, double* zprev_dev) {
    if (!ctx || !z_dev || !zprev_dev) return ASB_ERR_ARG;
    asb_zr* s = ctx->zr;
    if (!s || !s->begun) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_zroll_state: no roll-out begun (asb_zroll_begin)");
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    const dim3 gz((unsigned)(s->ld / 64), (unsigned)s->rq, 3);
    hipLaunchKernelGGL(k_zr_out, gz, dim3(64), 0, ctx->stream, s->Z, (int)s->n_sel, (int)s->r, (int)s->rq, s->ld, z_dev);
    hipLaunchKernelGGL(k_zr_out, gz, dim3(64), 0, ctx->stream, s->Zp, (int)s->n_sel, (int)s->r, (int)s->rq, s->ld, zprev_dev);
    ASB_CHECK_LAUNCH(ctx);
    ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ASB_OK;
}

// test hook: the product kernel alone on host arrays.  r rows, w columns, n_seg <= 8 segments of contraction lengths klen[s]:
// M_host the segments' (3, r, klen[s]) one behind the other, X_host their (3, klen[s], w); base_host (3, r, w), or (3, r) with
// bcast; out_host (3, rq, ld) gets the WHOLE padded result (rq = r rounded up to 16, ld = w to 64): the padding comes back zero
extern "C" int asb_test_zroll_affine(asb_ctx* ctx, int64_t r, int64_t w, int64_t n_seg, const int64_t* klen, const double* M_host, const double* X_host,
                                     const double* base_host, int bcast, double* out_host) {
    if (!ctx || r < 1 || w < 1 || n_seg < 1 || n_seg > ZR_MAX_SEG || !klen || !M_host || !X_host || !base_host || !out_host) return ASB_ERR_ARG;
    if (r > 8192 || w > (1 << 22)) ASB_FAIL(ctx, ASB_ERR_LIMIT, "asb_test_zroll_affine: %lld rows, %lld columns", (long long)r, (long long)w);
    for (int64_t sgi = 0; sgi < n_seg; ++sgi)
        if (klen[sgi] < 1 || klen[sgi] > (1 << 16)) ASB_FAIL(ctx, ASB_ERR_ARG, "asb_test_zroll_affine: a contraction of length %lld", (long long)klen[sgi]);
    ASB_HIP(ctx, hipSetDevice(ctx->dev));
    const long long rq = (r + 15) / 16 * 16, ld = (w + 63) / 64 * 64;
    asb_tmp<double> dM[ZR_MAX_SEG], dX[ZR_MAX_SEG], dB, dO;
    ZrSegs segs = {};
    segs.n = (int)n_seg;
    int rc;
    const double *pm = M_host, *px = X_host;
    for (int sgi = 0; sgi < n_seg; ++sgi) {
        const long long k = klen[sgi], kp = (k + 3) / 4 * 4;
        std::vector<double> mt((size_t)3 * kp * rq, 0.0), xs((size_t)3 * kp * ld, 0.0);
        for (int d = 0; d < 3; ++d)
            for (long long j = 0; j < r; ++j)
                for (long long q = 0; q < k; ++q) mt[((size_t)d * kp + q) * rq + j] = pm[((size_t)d * r + j) * k + q];
        for (int d = 0; d < 3; ++d)
            for (long long q = 0; q < k; ++q)
                for (long long c = 0; c < w; ++c) xs[((size_t)d * kp + q) * ld + c] = px[((size_t)d * k + q) * w + c];
        if ((rc = asb_test_stage(ctx, mt.data(), mt.size(), 0, dM[sgi])) || (rc = asb_test_stage(ctx, xs.data(), xs.size(), 0, dX[sgi]))) return rc;
        ASB_HIP(ctx, hipStreamSynchronize(ctx->stream));      // (the staging vectors die here)
        segs.s[sgi] = ZrSeg{dM[sgi].get(), dX[sgi].get(), (int)kp, (int)kp, ld};
        pm += 3 * r * k, px += 3 * k * w;
    }
    std::vector<double> bs(bcast ? (size_t)3 * rq : (size_t)3 * rq * ld, 0.0);
    for (int d = 0; d < 3; ++d)
        for (long long j = 0; j < r; ++j) {
            if (bcast) bs[(size_t)d * rq + j] = base_host[(size_t)d * r + j];
            else
                for (long long c = 0; c < w; ++c) bs[((size_t)d * rq + j) * ld + c] = base_host[((size_t)d * r + j) * w + c];
        }
    if ((rc = asb_test_stage(ctx, bs.data(), bs.size(), 0, dB)) || (rc = asb_test_stage(ctx, nullptr, (size_t)3 * rq * ld, 0, dO))) return rc;
    zr_affine_launch(ctx, segs, (int)rq, dB.get(), bcast != 0, dO.get(), ld, 0, w);
    rc = hipGetLastError() == hipSuccess ? ASB_OK : ASB_ERR_HIP;
    return asb_test_finish(ctx, rc, dO.get(), out_host, (size_t)3 * rq * ld);
}
