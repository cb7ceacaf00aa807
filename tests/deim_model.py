"""Plain numpy.longdouble model of the interpolation-point kernels of csrc/asb_pod.hip (DEIM residual and loop, block
residual, squared row norms of S^T M), for tests/test_deim_model_cpu.py and tests/test_gpu_deim_kernels.py.

Nothing here carries an inverse from step to step: every k x k system of the DEIM loop is solved from scratch.

Error bounds.  A float64 dot product of T terms deviates from the exact one by at most T u sum|terms| (u = 2^-53, to first
order).  An energy sum_c r_c^2 of such dot products r_c, each with absolute sum S_c >= |r_c|, deviates by at most
2 (T + 1 + A) u sum_c S_c^2, where A counts the additions that join the squares.  `bound(T, s)` = 8 (T + 4) u s keeps a
factor of four over that for T + 4 >= T + 1 + A roundings in the chain; the kernels' chains are counted where it is used.
"""
import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53


def bound(terms, abs_sum):
    return 8.0 * (terms + 4) * U53 * np.asarray(abs_sum, dtype=np.float64)


def first_argmax(e):
    """index and value of the first largest entry, and the largest entry among the others (-inf for a single entry)"""
    e = np.asarray(e)
    i = int(np.argmax(e))
    rest = np.delete(e, i)
    return i, e[i], (rest.max() if rest.size else -np.inf)


# ---- DEIM residual of one vector ------------------------------------------------------------------------------------
def residual(comps, k, coef):
    """comps (K, n, 3), coef (3, k) or None at k = 0.  r (n, 3) = sum_{j<k} coef[i][j] V[e,j,i] - V[e,k,i], and S (n, 3) the
    sum of the absolute values of those k + 1 terms."""
    V = np.asarray(comps, dtype=LD)
    r = -V[k].copy()
    S = np.abs(V[k])
    if k > 0:
        c = np.asarray(coef, dtype=LD)
        r = r + np.einsum("ij,jei->ei", c, V[:k])
        S = S + np.einsum("ij,jei->ei", np.abs(c), np.abs(V[:k]))
    return r, S


def step(comps, k, coef):
    """dict: energy (n,), ebound (n,) (the float64 kernel's deviation, k + 4 roundings), idx, val, second, maxabs, abound"""
    r, S = residual(comps, k, coef)
    e = (r * r).sum(axis=1)
    eb = bound(k, (S * S).sum(axis=1))
    i, val, second = first_argmax(e)
    return dict(r=r, energy=e, ebound=eb, idx=i, val=val, second=second, maxabs=np.abs(r).max(),
                abound=float(bound(k, S.max())))


# ---- linear systems ------------------------------------------------------------------------------------------------------
def gauss_solve(A, b):
    """longdouble Gaussian elimination with partial pivoting and back substitution"""
    A = np.array(A, dtype=LD)
    x = np.array(b, dtype=LD)
    n = A.shape[0]
    for c in range(n):
        piv = c + int(np.argmax(np.abs(A[c:, c])))
        if A[piv, c] == 0:
            raise ZeroDivisionError("singular system at column %d" % c)
        if piv != c:
            A[[c, piv]] = A[[piv, c]]
            x[[c, piv]] = x[[piv, c]]
        f = A[c + 1:, c] / A[c, c]
        A[c + 1:, c:] -= f[:, None] * A[c, c:][None, :]
        x[c + 1:] -= f * x[c]
    for c in range(n - 1, -1, -1):
        x[c] = (x[c] - A[c, c + 1:] @ x[c + 1:]) / A[c, c]
    return x


GAUSS_MAX = 48          # above this size: refined_solve (the loop below costs K^4 / 4 longdouble operations otherwise)


def refined_solve(A, b):
    """The same solution for large systems: a fresh float64 LU with partial pivoting (LAPACK) of THIS matrix, then
    iterative refinement with the residual in longdouble until the corrections stop shrinking (at k cond(A) 2^-64, where
    longdouble elimination ends as well: ~1e-14 at k = 600 against the 6e-12 of the float64 loop).  Converges
    for cond(A) << 2^53 (the callers' systems: ~1e3); tests/test_deim_model_cpu.py compares it with gauss_solve."""
    import scipy.linalg as sla
    A = np.asarray(A, dtype=LD)
    b = np.asarray(b, dtype=LD)
    lu = sla.lu_factor(A.astype(np.float64))
    x = np.zeros(b.shape, dtype=LD)
    prev, sizes = np.inf, []
    for _ in range(12):
        d = sla.lu_solve(lu, (b - A @ x).astype(np.float64))
        x = x + d
        size = float(np.abs(d).max()) / float(np.abs(x).max())
        if size <= 1e-18 or (size <= 1e-13 and size > 0.25 * prev):        # at the level k cond(A) 2^-64 allows: done
            return x
        prev = size
        sizes.append(size)
    raise ArithmeticError("refined_solve did not converge: corrections %s" % sizes)


def solve(A, b):
    return gauss_solve(A, b) if A.shape[0] <= GAUSS_MAX else refined_solve(A, b)


# ---- the whole DEIM loop ---------------------------------------------------------------------------------------------------
def deim_loop(comps, float64_too=False):
    """comps (K, n, 3).  dict: Pt (K,), maxabs (K,) longdouble, gap (K,): (best - second) / best of the row energies of
    every step (1 for a single row), and, on request, maxabs64: the same loop's largest |r| with numpy.linalg.solve and
    float64 products (the reference's arithmetic) at the model's points."""
    V = np.asarray(comps, dtype=LD)
    V64 = np.asarray(comps, dtype=np.float64)
    K = V.shape[0]
    Pt, maxabs, gap, m64 = [], [], [], []
    for k in range(K):
        r = -V[k].copy()
        r64 = -V64[k].copy()
        for i in range(3):
            if k > 0:
                x = solve(V[:k, Pt, i].T, V[k, Pt, i])
                r[:, i] += x @ V[:k, :, i]
                if float64_too:
                    r64[:, i] += np.linalg.solve(V64[:k, Pt, i].T, V64[k, Pt, i]) @ V64[:k, :, i]
        i0, best, second = first_argmax((r * r).sum(axis=1))
        Pt.append(i0)
        maxabs.append(np.abs(r).max())
        m64.append(np.abs(r64).max())
        gap.append((best - second) / best if np.isfinite(second) and best > 0 else LD(1))
    out = dict(Pt=np.array(Pt, dtype=np.int64), maxabs=np.array(maxabs, dtype=LD), gap=np.array(gap, dtype=LD))
    if float64_too:
        out["maxabs64"] = np.array(m64)
    return out


# ---- block residual ------------------------------------------------------------------------------------------------------
def block_residual(comps, k, p, coef):
    """comps (K, n, 3), coef (3, k p, p) or None.  r (n, p, 3) = sum_{j < k p} coef[i][j][m] V[e,j,i] - V[e,k p+m,i], S alike"""
    V = np.asarray(comps, dtype=LD)
    kp = k * p
    blk = V[kp:kp + p].transpose(1, 0, 2)                      # (n, p, 3)
    r = -blk
    S = np.abs(blk)
    if kp > 0:
        c = np.asarray(coef, dtype=LD)
        r = r + np.einsum("ijm,jei->emi", c, V[:kp])
        S = S + np.einsum("ijm,jei->emi", np.abs(c), np.abs(V[:kp]))
    return r, S


def block_step(comps, k, p, coef, group):
    """arg-max over rows (group 1) or over constraints of p rows (group p): dict as `step`, energy per group"""
    r, S = block_residual(comps, k, p, coef)
    n = r.shape[0]
    e = (r * r).sum(axis=(1, 2)).reshape(n // group, group).sum(axis=1)
    eb = bound(k * p, (S * S).sum(axis=(1, 2)).reshape(n // group, group).sum(axis=1))
    i, val, second = first_argmax(e)
    return dict(r=r, S=S, energy=e, ebound=eb, idx=i, val=val, second=second, maxabs=np.abs(r).max(),
                abound=float(bound(k * p, S.max())))


# ---- squared row norms of S^T M ------------------------------------------------------------------------------------------
def _segment_sums(P, indptr):
    """sums of the rows of P over the CSR segments (empty segments give zero)"""
    out = np.zeros((indptr.shape[0] - 1,) + P.shape[1:], dtype=P.dtype)
    full = np.flatnonzero(np.diff(indptr) > 0)
    if full.size:
        out[full] = np.add.reduceat(P, indptr[:-1][full], axis=0)
    return out


def st_rows(indptr, indices, data, M, S=None, extra_terms=0):
    """Row v of S^T M for a CSR matrix and a dense M (rows, cols).  S: per-entry absolute sums of M when M is itself a sum of
    `extra_terms` float64 products (default |M|, an exact input).  dict: energy (nv,), amax (nv,), ebound, abound: the
    float64 kernel's deviation for a chain of nnz(v) + extra_terms products, the square, cols / 64 per-lane additions and
    the six steps of the wave sum."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    w = np.asarray(data, dtype=LD)
    M = np.asarray(M, dtype=LD)
    S = np.abs(M) if S is None else np.asarray(S, dtype=LD)
    acc = _segment_sums(w[:, None] * M[indices], indptr)
    A = _segment_sums(np.abs(w)[:, None] * S[indices], indptr)
    nnz = np.diff(indptr)
    chain = nnz + extra_terms + (M.shape[1] + 63) // 64 + 6
    return dict(acc=acc, energy=(acc * acc).sum(axis=1), amax=np.abs(acc).max(axis=1) if M.shape[1] else np.zeros(len(nnz)),
                ebound=bound(chain, (A * A).sum(axis=1)), abound=bound(nnz + extra_terms, A.max(axis=1)))


def st_rows_split(indptr, slots, data, M_own, M_halo, S_own=None, S_halo=None, extra_terms=0):
    """The same for the owned rows of a shard: slot s < n_own reads M_own[s], the others M_halo[s - n_own]"""
    M = np.concatenate([np.asarray(M_own, dtype=LD), np.asarray(M_halo, dtype=LD).reshape(-1, np.shape(M_own)[1])])
    S = None
    if S_own is not None:
        S = np.concatenate([np.asarray(S_own, dtype=LD), np.asarray(S_halo, dtype=LD).reshape(-1, np.shape(S_own)[1])])
    return st_rows(indptr, slots, data, M, S, extra_terms)
