"""Plain NumPy model of the constraint-basis chain (csrc/asb_pod.hip, asb_orth_gram and the row combinations of
csrc/asb_linalg.hip, k_comps_post of csrc/asb_deflate.hip), one function per device phase, on what the device holds: the
snapshots X as (F, n, 3), a basis C as (K, n, 3) whose flat rows are the (3 n)-vectors r = 3 v + l, B as (K, F).
tests/test_pod_model_cpu.py holds the model against LAPACK; tests/test_gpu_pod_phases.py compares every device phase with the
model run in numpy.longdouble on the device's own inputs.

Every function takes ``dtype`` (numpy.float64 or numpy.longdouble) and computes in it from its first operation on; nothing
leaves that type (no LAPACK, no BLAS in longdouble: the Cholesky factor, its inverse and the one-sided Jacobi are written here).
"""
import numpy as np

from splocs_model import deviation          # noqa: F401  (relative Frobenius norm, largest entry over largest entry)


def flat(C, dtype=np.float64):
    """(K, n, 3) -> (K, 3 n): the rows the device stores"""
    C = np.asarray(C, dtype=dtype)
    return C.reshape(C.shape[0], -1)


def rows(X, dtype=np.float64):
    """the snapshots (F, n, 3) as the matrix A (3 n, F) of the POD: A[3 v + l][f] = X[f][v][l]"""
    return flat(X, dtype).T


def unrows(A, n):
    """A (3 n, F) back to (F, n, 3)"""
    return np.ascontiguousarray(A.T).reshape(A.shape[1], n, 3)


# ------------------------------------------------------------------------------------------------ element-wise phases
def affine(X, inv_scale, mean, rowscale, dtype=np.float64):
    """k_affine_rows: (X * inv_scale + mean) * rowscale; mean (n, 3) or None, rowscale (n,) per vertex or None"""
    Y = np.asarray(X, dtype=dtype) * dtype(inv_scale)
    if mean is not None:
        Y = Y + np.asarray(mean, dtype=dtype)[None]
    if rowscale is not None:
        Y = Y * np.asarray(rowscale, dtype=dtype)[None, :, None]
    return Y


def affine_terms(X, inv_scale, mean, rowscale):
    """sum of the magnitudes of affine's terms per entry (longdouble): what its rounding errors are relative to"""
    LD = np.longdouble
    T = np.abs(np.asarray(X, dtype=LD) * LD(inv_scale))
    if mean is not None:
        T = T + np.abs(np.asarray(mean, dtype=LD))[None]
    if rowscale is not None:
        T = T * np.abs(np.asarray(rowscale, dtype=LD))[None, :, None]
    return T


def comps_post(C, unscale, psf, mean, inv_mass, dtype=np.float64):
    """k_comps_post: C / psf + mean when unscale, then times inv_mass per vertex when given"""
    Y = np.asarray(C, dtype=dtype)
    if unscale:
        Y = Y / dtype(psf) + np.asarray(mean, dtype=dtype)[None]
    if inv_mass is not None:
        Y = Y * np.asarray(inv_mass, dtype=dtype)[None, :, None]
    return Y


def comps_post_terms(C, unscale, psf, mean, inv_mass):
    LD = np.longdouble
    T = np.abs(np.asarray(C, dtype=LD))
    if unscale:
        T = T / abs(LD(psf)) + np.abs(np.asarray(mean, dtype=LD))[None]
    if inv_mass is not None:
        T = T * np.abs(np.asarray(inv_mass, dtype=LD))[None, :, None]
    return T


# ------------------------------------------------------------------------------------------------ Gram matrices and CholeskyQR
def slice_grams(C, dtype=np.float64):
    """(3, K, K): G[l] = C[:, :, l] C[:, :, l]^T (asb_orth_gram)"""
    C = np.asarray(C, dtype=dtype)
    return np.stack([C[:, :, l] @ C[:, :, l].T for l in range(3)])


def joint_gram(C, dtype=np.float64):
    """(K, K): the Gram matrix of the (3 n)-vectors, summed over the slices in k_sum3's order"""
    G = slice_grams(C, dtype)
    return (G[0] + G[1]) + G[2]


def cholesky(G, dtype=np.float64):
    """unblocked lower Cholesky factor, column by column; ValueError on a pivot that is not positive (k_chol_tinv's refusal)"""
    L = np.array(G, dtype=dtype)
    K = L.shape[0]
    for j in range(K):
        d = L[j, j]
        if not d > 0:
            raise ValueError("rank deficient: pivot %d is %r" % (j, float(d)))
        sq = np.sqrt(d)
        L[j, j] = sq
        L[j + 1:, j] = L[j + 1:, j] / sq
        L[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
    return np.tril(L)


def lower_inverse(L, dtype=np.float64):
    """T = L^-1 by forward substitution, row by row"""
    K = L.shape[0]
    T = np.zeros((K, K), dtype=dtype)
    for i in range(K):
        e = np.zeros(K, dtype=dtype)
        e[i] = 1
        T[i] = (e - L[i, :i] @ T[:i]) / L[i, i]
    return T


def chol_qr(C, G, joint, dtype=np.float64):
    """one CholeskyQR pass with the Gram matrices G (3, K, K) the caller read back: with Tt = L^-T the new component j is
    sum_i comps_i Tt[i][j] = row j of L^-1 C, per coordinate slice (joint false) or with the one factor of (G0 + G1) + G2
    for all three (joint true)"""
    C = np.asarray(C, dtype=dtype)
    G = np.asarray(G, dtype=dtype)
    out = np.empty_like(C)
    if joint:
        T = lower_inverse(cholesky((G[0] + G[1]) + G[2], dtype), dtype)
        for l in range(3):
            out[:, :, l] = T @ C[:, :, l]
    else:
        for l in range(3):
            out[:, :, l] = lower_inverse(cholesky(G[l], dtype), dtype) @ C[:, :, l]
    return out


def orth_defect(C, joint):
    """(|Q Q^T - I|_F / sqrt(K), largest entry of |Q Q^T - I|) in longdouble, the worst of the three slices or of the joint
    basis"""
    LD = np.longdouble
    Gs = joint_gram(C, LD)[None] if joint else slice_grams(C, LD)
    K = Gs.shape[1]
    D = Gs - np.eye(K, dtype=LD)[None]
    return float(np.sqrt((D * D).sum(axis=(1, 2)).max() / K)), float(np.abs(D).max())


# ------------------------------------------------------------------------------------------------ the POD phases
def basis(X, V, lam, K, dtype=np.float64):
    """comps[k] = A V[:, k] / sqrt(max(lam[k], 0)) for k < K (asb_pod_basis, asb_pod_basis_dev); a lam <= 0 divides by zero"""
    A = rows(X, dtype)
    V = np.asarray(V, dtype=dtype)[:, :K]
    s = np.sqrt(np.maximum(np.asarray(lam, dtype=dtype)[:K], dtype(0)))
    with np.errstate(divide="ignore", invalid="ignore"):
        U = (A @ V) / s[None]
    return np.ascontiguousarray(U.T).reshape(K, -1, 3)


def project(C, X, dtype=np.float64):
    """B = Q A (K, F): B[k][f] = sum_r C[k][r] A[r][f]  (asb_pod_project)"""
    return flat(C, dtype) @ rows(X, dtype)


def _round_robin(n2):
    """the n2 - 1 rounds of n2 / 2 disjoint pairs (n2 even) that visit every pair once: the parallel cyclic order"""
    idx = list(range(n2))
    for _ in range(n2 - 1):
        yield np.array(idx[:n2 // 2]), np.array(idx[n2 // 2:][::-1])
        idx = [idx[0], idx[-1]] + idx[1:-1]


def jacobi_rows(B, dtype=np.float64, max_sweeps=60):
    """cyclic one-sided (Hestenes) Jacobi on the rows of B (K, F): returns (R, J) with R = J B, the rows of R mutually
    orthogonal (unsorted) and J orthogonal.  Pairs within a round are disjoint and rotated at once."""
    R = np.array(B, dtype=dtype)
    K = R.shape[0]
    J = np.eye(K, dtype=dtype)
    if K == 1:
        return R, J
    tol = 4 * np.finfo(dtype).eps
    n2 = K + (K & 1)
    for _ in range(max_sweeps):
        rotated = 0
        for p, q in _round_robin(n2):
            live = (p < K) & (q < K)
            p, q = p[live], q[live]
            a, b, g = (R[p] * R[p]).sum(axis=1), (R[q] * R[q]).sum(axis=1), (R[p] * R[q]).sum(axis=1)
            act = np.abs(g) > tol * np.sqrt(a * b)
            if not act.any():
                continue
            rotated += int(act.sum())
            p, q, a, b, g = p[act], q[act], a[act], b[act], g[act]
            zeta = (b - a) / (2 * g)
            t = np.where(zeta >= 0, dtype(1), dtype(-1)) / (np.abs(zeta) + np.sqrt(1 + zeta * zeta))
            c = 1 / np.sqrt(1 + t * t)
            s = c * t
            for M in (R, J):
                Mp, Mq = M[p].copy(), M[q].copy()
                M[p] = c[:, None] * Mp - s[:, None] * Mq
                M[q] = s[:, None] * Mp + c[:, None] * Mq
        if not rotated:
            return R, J
    raise ValueError("one-sided Jacobi: no convergence in %d sweeps" % max_sweeps)


def rotate_rows(B, dtype=np.float64):
    """the small SVD of asb_pod_rotate: (S descending, U, rows) -- row r of U is the row combination that gives the r-th left
    singular vector of B, rows[r] = U[r] B = sigma_r v_r^T"""
    R, J = jacobi_rows(B, dtype)
    S = np.sqrt((R * R).sum(axis=1))
    order = np.argsort(-S, kind="stable")
    return S[order], J[order], R[order]


def rotate(C, B, dtype=np.float64, small=None):
    """asb_pod_rotate: (S, U, rows, basis) with basis[r] = sum_i U[r][i] C[i]; ``small``: rotate_rows(B, dtype) when the caller
    has it already"""
    S, U, R = rotate_rows(B, dtype) if small is None else small
    return S, U, R, (U @ flat(C, dtype)).reshape(np.asarray(C).shape)


def power(X, B_rot, S, dtype=np.float64):
    """asb_pod_power: row r of the new basis is A (B_rot[r] / S[r]^2), and 0 where S[r] == 0 (B_rot in S's order)"""
    A = rows(X, dtype)
    B_rot, S = np.asarray(B_rot, dtype=dtype), np.asarray(S, dtype=dtype)
    Vn = np.zeros_like(B_rot)
    ok = S > 0
    Vn[ok] = B_rot[ok] / (S[ok] * S[ok])[:, None]
    return (Vn @ A.T).reshape(B_rot.shape[0], -1, 3)


def deflate(X, C_keep, B_keep, dtype=np.float64):
    """asb_pod_deflate_begin: A - C_keep^T B_keep, returned as (F, n, 3)"""
    A = rows(X, dtype) - flat(C_keep, dtype).T @ np.asarray(B_keep, dtype=dtype)
    return unrows(A, np.asarray(X).shape[1])


def align_signs(got, ref):
    """got's rows with the sign that makes <got[r], ref[r]> >= 0 (singular vectors are defined up to sign)"""
    got = np.asarray(got)
    g2, r2 = got.reshape(got.shape[0], -1), np.asarray(ref, dtype=np.longdouble).reshape(got.shape[0], -1)
    sgn = np.where((g2.astype(np.longdouble) * r2).sum(axis=1) < 0, -1.0, 1.0)
    return got * sgn.reshape((-1,) + (1,) * (got.ndim - 1)).astype(got.dtype)
