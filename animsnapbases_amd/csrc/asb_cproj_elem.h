// "Project F": the second half of the strain and deformation-gradient projections of asb_cproj.hip, as functions of the
// deformation gradient F, the clamp and the kind alone -- host and device, so that the kernels (k_cproj, k_cproj_em), the
// host probe and the device probe of asb_test_cproj_project_* run the same text (tests/test_cproj_model_cpu.py,
// tests/test_gpu_cproj_edges.py).
//
// SVD: one-sided (Hestenes) Jacobi on F itself -- column pairs of A = F V are rotated until orthogonal, the column norms are
// the singular values, u_i = a_i / sigma_i -- with a fixed bound on the sweeps and an early out.  F^T F is never formed.
// Every result is a function of F: sum_i g(sigma_i) u_i v_i^T does not depend on the order or signs the sweeps end with.
//
//   scale   F is first multiplied by the power of two that brings max|f_ij| into [0.5, 1): exact, and the squared norms, the
//           products of two of them and the determinant can then neither overflow nor flush to zero.  The singular values are
//           multiplied back before the clamp.  F = 0 gives U = V = I, sigma = 0.
//   rank    after the sweeps a column with |a_j| <= CP_RANK_TOL max|f_ij| is null: sigma_j = 0 exactly, and the column is
//           never normalised into U (what the sweeps leave of a vanished column is rounding noise of norm 1e-16 sigma_1
//           without a direction; rotating it against the others moves them by 1e-32, and such an F runs to the bound on the
//           sweeps).  max|f_ij| <= sigma_1 <= 3 max|f_ij|, so the threshold is 0.33 .. 1e-12 sigma_1.  The test is made once,
//           on the converged columns: a column on its way to zero passes through every size and still carries signal.
//   U       is completed to an orthogonal matrix with det U = +1 relative to its non-null columns: one null column is the
//           cross product of the other two in cyclic order, two null columns are an orthonormal complement of the third.
//           V is a product of plane rotations, det V = +1 always, so this is the SVD with det U det V = +1, the non-inverted
//           one.  No column of V is ever copied into U.
#pragma once
#include <math.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#define __device__
#endif
#ifndef __forceinline__
#define __forceinline__ inline
#endif
#endif

#define CP_SWEEPS 12        // bound on the Jacobi sweeps (3 x 3 converges in 4 - 6)
#define CP_TOL 4.440892098500626e-16        // columns count as orthogonal at |a_p . a_q| <= CP_TOL |a_p| |a_q|
#define CP_RANK_TOL 1.0e-12 // a column is null at |a_j| <= CP_RANK_TOL max|f_ij| (procrustes_rot: the same figure)

enum { CP_EDGE = 0, CP_TRI = 1, CP_TET_STRAIN = 2, CP_TET_DEFGRAD = 3, CP_BEND = 4 };

// one Jacobi rotation of the columns p, q of A (N rows) and of V (N rows): true when it rotated
template <int N>
__host__ __device__ __forceinline__ bool cp_rotate(double (&A)[N][N], double (&V)[N][N], int p, int q) {
    double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        al = fma(A[i][p], A[i][p], al);
        be = fma(A[i][q], A[i][q], be);
        ga = fma(A[i][p], A[i][q], ga);
    }
    if (!(fabs(ga) > CP_TOL * sqrt(al * be))) return false;         // (entries below 1 after the scaling: no overflow)
    const double zeta = (be - al) / (2.0 * ga);
    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double ap = A[i][p], aq = A[i][q], vp = V[i][p], vq = V[i][q];
        A[i][p] = c * ap - s * aq;
        A[i][q] = s * ap + c * aq;
        V[i][p] = c * vp - s * vq;
        V[i][q] = s * vp + c * vq;
    }
    return true;
}

// A *= 2^-e with 2^(e-1) <= max|a_ij| < 2^e, V = I; returns 2^e (1 for A = 0); nul2 = the squared norm at and below which a
// column of the scaled matrix is null, (CP_RANK_TOL max|a_ij|)^2
template <int N>
__host__ __device__ __forceinline__ double cp_scale(double (&A)[N][N], double (&V)[N][N], double& nul2) {
    double mx = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) {
            V[i][j] = i == j ? 1.0 : 0.0;
            mx = fmax(mx, fabs(A[i][j]));
        }
    nul2 = 0.0;
    if (!(mx > 0.0)) return 1.0;
    int e;
    frexp(mx, &e);
    if (e < -1000) e = -1000;                       // (2^-e must stay finite: entries below 2^-1000 are scaled by 2^1000 only)
    const double down = ldexp(1.0, -e);
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) A[i][j] *= down;
    mx *= down * CP_RANK_TOL;
    nul2 = mx * mx;
    return ldexp(1.0, e);
}

__host__ __device__ __forceinline__ double cp_det3(const double (&M)[3][3]) {
    return M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
           M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
}

// F = U diag(sig) V^T with det U det V = +1 on null columns (the header's rules).  In: A = F; out: A = U, V, sig (any order),
// inverted = no column is null and det F < 0 (a deficient F has det F = 0, whatever sign its float64 residue has: not inverted)
__host__ __device__ __forceinline__ void cp_svd3(double (&A)[3][3], double (&V)[3][3], double (&sig)[3], bool& inverted) {
    double nul2;
    const double up = cp_scale<3>(A, V, nul2);
    const double det = cp_det3(A);
    for (int sw = 0; sw < CP_SWEEPS; ++sw) {
        bool r = cp_rotate<3>(A, V, 0, 1);
        r |= cp_rotate<3>(A, V, 0, 2);
        r |= cp_rotate<3>(A, V, 1, 2);
        if (!r) break;
    }
    bool nul[3];
    int nn = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double n2 = A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j];
        nul[j] = !(n2 > nul2);
        if (nul[j]) {
            sig[j] = 0.0;
            ++nn;
        } else {
            const double n = sqrt(n2), inv = 1.0 / n;
            sig[j] = n * up;
            A[0][j] *= inv, A[1][j] *= inv, A[2][j] *= inv;
        }
    }
    inverted = nn == 0 && det < 0.0;
    if (nn == 0) return;                            // full rank: nothing to complete
    if (nn == 3) {                                  // F = 0
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) A[i][j] = i == j ? 1.0 : 0.0;
    }
    // (the column indices below are compile-time constants under the unrolling: A stays in registers)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (nn != 2 || nul[k]) continue;            // rank 1: u_b = (u_k x e) / |u_k x e| for the axis e that u_k has least of,
        const int b = (k + 1) % 3, c = (k + 2) % 3; // u_c = u_k x u_b; (k, b, c) cyclic, so det U = +1
        const double x0 = A[0][k], x1 = A[1][k], x2 = A[2][k];
        const double m0 = fabs(x0), m1 = fabs(x1), m2 = fabs(x2);
        const int ax = (m0 <= m1 && m0 <= m2) ? 0 : (m1 <= m2 ? 1 : 2);
        const double e0 = ax == 0 ? 1.0 : 0.0, e1 = ax == 1 ? 1.0 : 0.0, e2 = ax == 2 ? 1.0 : 0.0;
        double w0 = x1 * e2 - x2 * e1, w1 = x2 * e0 - x0 * e2, w2 = x0 * e1 - x1 * e0;
        const double inv = 1.0 / sqrt(w0 * w0 + w1 * w1 + w2 * w2);
        w0 *= inv, w1 *= inv, w2 *= inv;
        A[0][b] = w0, A[1][b] = w1, A[2][b] = w2;
        A[0][c] = x1 * w2 - x2 * w1;
        A[1][c] = x2 * w0 - x0 * w2;
        A[2][c] = x0 * w1 - x1 * w0;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (nn != 1 || !nul[j]) continue;           // rank 2: u_j = u_a x u_b, (j, a, b) cyclic
        const int a = (j + 1) % 3, b = (j + 2) % 3;
        A[0][j] = A[1][a] * A[2][b] - A[2][a] * A[1][b];
        A[1][j] = A[2][a] * A[0][b] - A[0][a] * A[2][b];
        A[2][j] = A[0][a] * A[1][b] - A[1][a] * A[0][b];
    }
}

__host__ __device__ __forceinline__ double cp_clip(double s, double lo, double hi) { return fmin(fmax(s, lo), hi); }

// tris_strain (:411-425): Fhat = U clip(sigma) V^T of the 2 x 2 F; the caller applies (P Fhat)^T
__host__ __device__ __forceinline__ void cp_project_tri(const double (&F)[2][2], double smin, double smax, double (&Fh)[2][2]) {
    double A[2][2] = {{F[0][0], F[0][1]}, {F[1][0], F[1][1]}}, V[2][2], nul2;
    const double up = cp_scale<2>(A, V, nul2);
    for (int sw = 0; sw < CP_SWEEPS; ++sw)
        if (!cp_rotate<2>(A, V, 0, 1)) break;
    double sg[2];
    bool nul[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const double n2 = A[0][j] * A[0][j] + A[1][j] * A[1][j];
        nul[j] = !(n2 > nul2);
        sg[j] = 0.0;
        if (!nul[j]) {
            const double n = sqrt(n2), inv = 1.0 / n;
            sg[j] = n * up;
            A[0][j] *= inv, A[1][j] *= inv;
        }
    }
    if (nul[0] && nul[1]) {                         // F = 0
        A[0][0] = 1.0, A[1][0] = 0.0, A[0][1] = 0.0, A[1][1] = 1.0;
    } else if (nul[1]) {                            // the quarter turn that makes det U = +1 (det V = +1 always)
        A[0][1] = -A[1][0], A[1][1] = A[0][0];
    } else if (nul[0]) {
        A[0][0] = A[1][1], A[1][0] = -A[0][1];
    }
    const double c0 = cp_clip(sg[0], smin, smax), c1 = cp_clip(sg[1], smin, smax);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) Fh[i][j] = c0 * A[i][0] * V[j][0] + c1 * A[i][1] * V[j][1];
}

// tets_strain (:538-554): r = U diag(c) V^T row-major, c = clip(sigma), the SMALLEST one negated on an inverted element;
// tets_deformation_gradient (:673-687): r = R^T, R = U V^T with its third COLUMN negated where det R < 0
template <int KIND>
__host__ __device__ __forceinline__ void cp_project_tet(const double (&F)[3][3], double smin, double smax, double (&r)[9]) {
    double A[3][3], V[3][3], sg[3];
    bool inverted;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) A[i][j] = F[i][j];
    cp_svd3(A, V, sg, inverted);
    if (KIND == CP_TET_STRAIN) {
        int lo = sg[1] < sg[0] ? 1 : 0;
        if (sg[2] <= sg[lo]) lo = 2;
        double c[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            c[j] = cp_clip(sg[j], smin, smax);
            if (inverted && j == lo) c[j] = -c[j];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) r[3 * i + j] = c[0] * A[i][0] * V[j][0] + c[1] * A[i][1] * V[j][1] + c[2] * A[i][2] * V[j][2];
    } else {
        double R[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) R[i][j] = A[i][0] * V[j][0] + A[i][1] * V[j][1] + A[i][2] * V[j][2];
        if (cp_det3(R) < 0.0) R[0][2] = -R[0][2], R[1][2] = -R[1][2], R[2][2] = -R[2][2];      // (:684-685): third COLUMN of R
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) r[3 * i + j] = R[j][i];                                  // (:687) R^T
    }
}
