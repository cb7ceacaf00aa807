"""Plain NumPy model of the SPLOCS refinement (csrc/asb_splocs.hip), one function per phase, in the LIBRARY's formulation: the
residual is never formed, the weight sweep works from P = X C^T and M = C C^T, the ADMM applies an explicit (G + rho I)^-1 and
the objective comes from <W, P> and <G, M>.  tests/test_splocs_model_cpu.py chains the phases and shows that they are the
algorithm of oracle.asb_oracle.splocs_glob_optimization (posComponents.py:132-189 of the reference); the GPU tests compare each
device phase with the model run in numpy.longdouble on what the device holds.

Every function takes ``dtype`` (numpy.float64 or numpy.longdouble) and computes in it from its first operation on; nothing
leaves that type (no LAPACK, no BLAS in longdouble: the K x K inverse is an explicit Cholesky factorisation written here).

One deliberate difference from the reference: the group soft threshold takes ``len == 0 -> z = 0`` (the kernels' documented
convention, k_admm_prox / k_admm_fused).  NumPy's formula ``x * max(0, 1 - beta Lambda / len)`` gives NaN where Lambda = 0 and
x = 0 (0 / 0) and 0 * (-inf -> 0) = 0 where Lambda > 0; the reference never meets the first on real data, the model and the
kernels define both as 0.

Shapes: X (F, n, 3), C and U (K, n, 3), W (F, K), Lambda (K, n), P (F, K), M and G (K, K), c (K, 3 n).
"""
import numpy as np

DEAD = 1.e-8            # a component with |C_k|^2 <= DEAD is zero everywhere: zero activation (:147-150)


def _flat(A, dtype):
    A = np.asarray(A, dtype=dtype)
    return A.reshape(A.shape[0], -1)


def gram(X, C, dtype=np.float64):
    """(P = X_flat C_flat^T, M = C_flat C_flat^T, |X|^2)"""
    Xf, Cf = _flat(X, dtype), _flat(C, dtype)
    return Xf @ Cf.T, Cf @ Cf.T, (Xf * Xf).sum()


def project_weight(x):
    """posComponents.py:52-58: clamp at 0, divide by the maximum unless it is 0"""
    x = np.maximum(x.dtype.type(0), x)
    top = x.max() if x.size else x.dtype.type(0)
    return x if top == 0 else x / top


def weights(W, P, M, dtype=np.float64):
    """The sweep of :144-156 with the residual eliminated: opt_k = (P[:, k] - W M[:, k]) / M[k, k] + W[:, k], sequentially in k
    (W M[:, k] sees the columns already updated); a dead column becomes zero.  Returns the new W."""
    W = np.array(W, dtype=dtype)
    P, M = np.asarray(P, dtype=dtype), np.asarray(M, dtype=dtype)
    for k in range(W.shape[1]):
        nk = M[k, k]
        if nk <= DEAD:
            W[:, k] = 0
            continue
        W[:, k] = project_weight((P[:, k] - W @ M[:, k]) / nk + W[:, k])
    return W


def centres(C, v0=0, dtype=np.float64):
    """per component v0 + the first vertex of largest |C_k[v]|^2 (:161), and that value"""
    e = (np.asarray(C, dtype=dtype) ** 2).sum(axis=2)
    idx = e.argmax(axis=1)                      # numpy: the first of equal maxima
    return v0 + idx.astype(np.int64), e[np.arange(e.shape[0]), idx]


def cholesky_inverse(A):
    """A^-1 of a symmetric positive definite A through A = L L^T, in A's own type: Y = L^-1 by forward substitution,
    A^-1 = Y^T Y."""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite")
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Y = np.zeros_like(A)
    for i in range(n):
        r = -(L[i, :i] @ Y[:i])
        r[i] += 1
        Y[i] = r / L[i, i]
    return Y.T @ Y


def prox_l1l2(Lambda, x, beta):
    """group soft threshold over xyz (:252-256) with len == 0 -> 0 (see the module docstring)"""
    one, zero = x.dtype.type(1), x.dtype.type(0)
    ln = np.sqrt((x * x).sum(axis=-1))
    safe = np.where(ln > 0, ln, one)
    shrink = np.where(ln > 0, np.maximum(zero, one - beta * Lambda / safe), zero)
    return x * shrink[..., None]


def admm(X, W, C, U, Lambda, rho, n_iter, dtype=np.float64):
    """:168-181.  Z = C; G = W^T W; c = W^T X; Ginv = (G + rho I)^-1; n_iter times: C = Ginv (c + rho (Z - U)),
    Z = prox(Lambda, C + U, 1 / rho), U += C - Z; the result is C = Z.  Returns dict(C, U, G, Ginv, c)."""
    W = np.asarray(W, dtype=dtype)
    Xf = _flat(X, dtype)
    Z = np.array(C, dtype=dtype)
    U = np.array(U, dtype=dtype)
    Lambda = np.asarray(Lambda, dtype=dtype)
    K = W.shape[1]
    rho = dtype(rho)
    G = W.T @ W
    c = W.T @ Xf
    Ginv = cholesky_inverse(G + rho * np.eye(K, dtype=dtype))
    beta = dtype(1) / rho
    for _ in range(n_iter):
        Cn = (Ginv @ (c + rho * (Z - U).reshape(c.shape))).reshape(Z.shape)
        Z = prox_l1l2(Lambda, Cn + U, beta)
        U = U + Cn - Z
    return dict(C=Z, U=U, G=G, Ginv=Ginv, c=c)


def objective(W, G, P, M, Lambda, C, dtype=np.float64):
    """(<W, P>, <G, M>, sum Lambda |C_v|) with P, M of the NEW C: |X - W C|^2 = |X|^2 - 2 <W, P> + <G, M>   (:183-186)"""
    a = [np.asarray(v, dtype=dtype) for v in (W, G, P, M, Lambda, C)]
    return (a[0] * a[2]).sum(), (a[1] * a[3]).sum(), (a[4] * np.sqrt((a[5] * a[5]).sum(axis=2))).sum()


def lambda_from_fields(phi, lam, dmin, dmax, dtype=np.float64):
    """Lambda = lam (clip(phi, dmin, dmax) - dmin) / (dmax - dmin)   (:162-165, utils/support.py:61-64)"""
    phi = np.asarray(phi, dtype=dtype)
    dmin, dmax, lam = dtype(dmin), dtype(dmax), dtype(lam)
    return lam * ((np.minimum(np.maximum(phi, dmin), dmax) - dmin) / (dmax - dmin))


def deviation(a, b):
    """(relative Frobenius norm of a - b, largest entry of |a - b| over the largest entry of |b|), as float64; both 0 where
    b is zero and a equals it, inf where b is zero and a is not"""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    d = a - b
    if not b.size:
        return 0.0, 0.0
    nb, mb = np.sqrt((b * b).sum()), np.abs(b).max()
    nd, md = np.sqrt((d * d).sum()), np.abs(d).max()
    return float(nd / nb) if nb > 0 else (0.0 if nd == 0 else np.inf), float(md / mb) if mb > 0 else (0.0 if md == 0 else np.inf)
