"""Plain NumPy model of the heat method on WHAT THE DEVICE HOLDS (csrc/asb_geodesic.hip): the float64 operators that
GeodesicDistanceComputation.prepare() assembles -- A_heat = A - tL, L, the gradient G (3M x N) and the divergence D (N x 3M) --
cast to a chosen dtype, and then, for a source s,

    1. u = A_heat^-1 e_s
    2. X = -G u / |G u| per face
    3. b = D X
    4. y = (-L + (gamma / n) 1 1^T)^-1 (b - mean b),   gamma = mean diag(-L)
    5. phi = max(y) - y

In numpy.float64 the two systems go through numpy.linalg.solve on dense arrays: the yardstick.  In numpy.longdouble nothing leaves
that type (NumPy has no longdouble LAPACK): both systems are factorised by the band Cholesky written here, the sparse heat matrix in
a reverse Cuthill-McKee numbering, the gauge-fixed Laplacian of step 4 as the dense matrix it is.  Above DENSE_LIMIT vertices the
longdouble model replaces step 4's dense matrix by the Laplacian with ONE grounded vertex, (-L + gamma e_g e_g^T) w = b - mean b,
y = w - mean w: the right-hand side is orthogonal to the constants, so w solves the singular system exactly, and the mean-free
solution of the singular system is what the gauge-fixed matrix returns (it maps 1 to gamma 1 and leaves 1's complement to -L).
(In exact arithmetic on an exactly singular L.  The rows of the float64 L sum to zero up to a few eps of their diagonal only, so
on the operators as held the two forms differ by cond(-L) times that: the dense mode's gauge form, the slab mode's grounded form
and the sparse mode's singular system are three such forms, and the tolerance of the GPU tests covers their spread.)
G and D stay sparse (three entries per row of G); their products are formed in the dtype with a fixed order.
"""
import numpy as np
from scipy import sparse
from scipy.sparse.csgraph import reverse_cuthill_mckee

from splocs_model import deviation          # noqa: F401  (relative Frobenius norm, largest entry over largest entry)

LD = np.longdouble
DENSE_LIMIT = 1024


# ------------------------------------------------------------------------------------------------ band Cholesky, any dtype
def band_from_dense(A):
    """lower band storage W[j, d] = A[j + d, j] of a symmetric matrix (full bandwidth)"""
    n = A.shape[0]
    W = np.zeros((n, n), dtype=A.dtype)
    for d in range(n):
        W[:n - d, d] = np.diagonal(A, -d)
    return W


def band_from_sparse(S, dtype):
    """lower band storage of a symmetric sparse matrix (values cast to dtype, duplicates summed in it)"""
    C = sparse.coo_matrix(S)
    C.sum_duplicates()
    keep = C.row >= C.col
    r, c, v = C.row[keep], C.col[keep], C.data[keep].astype(dtype)
    bw = int((r - c).max()) if r.size else 0
    W = np.zeros((S.shape[0], bw + 1), dtype=dtype)
    W[c, r - c] = v
    return W


def band_cholesky(W):
    """in place: W[j, d] = L[j + d, j] of A = L L^T (right-looking; the trailing update of column j touches the triangle
    W[j + p, q - p], 1 <= p <= q <= m, which is one strided view of the band)"""
    n, w = W.shape
    bw = w - 1
    item = W.itemsize
    for j in range(n):
        d = W[j, 0]
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite")
        d = np.sqrt(d)
        W[j, 0] = d
        m = min(bw, n - 1 - j)
        if m == 0:
            continue
        W[j, 1:m + 1] /= d
        c = W[j, 1:m + 1]
        if bw > 0:
            view = np.lib.stride_tricks.as_strided(W[j + 1:, :], shape=(m, m), strides=(bw * item, item))
            view -= np.triu(np.outer(c, c))         # (below the diagonal the view aliases other band entries: they get - 0)
    return W


def band_solve(W, B):
    """A^-1 B from the factor of band_cholesky; B (n, k)"""
    n, w = W.shape
    bw = w - 1
    Y = np.array(B, dtype=W.dtype)
    for j in range(n):
        Y[j] /= W[j, 0]
        m = min(bw, n - 1 - j)
        if m:
            Y[j + 1:j + m + 1] -= np.outer(W[j, 1:m + 1], Y[j])
    for j in range(n - 1, -1, -1):
        m = min(bw, n - 1 - j)
        if m:
            Y[j] -= W[j, 1:m + 1] @ Y[j + 1:j + m + 1]
        Y[j] /= W[j, 0]
    return Y


def cholesky_inverse(A):
    """A^-1 of a symmetric positive definite A in A's own type (the band routines at full bandwidth)"""
    return band_solve(band_cholesky(band_from_dense(np.array(A))), np.eye(A.shape[0], dtype=A.dtype))


class _SparseSPD(object):
    """a sparse SPD matrix factorised in longdouble in a bandwidth-reducing numbering"""

    def __init__(self, S, dtype):
        S = sparse.csr_matrix(S)
        self.perm = np.asarray(reverse_cuthill_mckee(S, symmetric_mode=True), dtype=np.int64)
        self.W = band_cholesky(band_from_sparse(S[self.perm][:, self.perm], dtype))

    def solve(self, B):
        out = np.empty_like(B)
        out[self.perm] = band_solve(self.W, B[self.perm])
        return out


def _csr_times(S, X, dtype):
    """S X with a float64 CSR matrix cast to dtype, rows summed in storage order"""
    S = sparse.csr_matrix(S)
    S.sort_indices()
    assert (np.diff(S.indptr) > 0).all(), "an empty row"
    return np.add.reduceat(S.data.astype(dtype)[:, None] * X[S.indices], S.indptr[:-1], axis=0)


class HeatModel(object):
    """model = HeatModel(A_heat, L, G, D, dtype); model.fields(sources) -> (len(sources), n) distances in dtype"""

    def __init__(self, A_heat, L, G, D, dtype=np.float64):
        self.dtype = dtype
        self.n = n = A_heat.shape[0]
        self.G, self.D = sparse.csr_matrix(G), sparse.csr_matrix(D)
        negL = sparse.csr_matrix(-L)
        self.gamma = negL.diagonal().astype(dtype).sum() / dtype(n)
        self.grounded = False
        if dtype is np.float64:
            A = np.asarray(A_heat.todense(), dtype=np.float64)
            P = np.asarray(negL.todense(), dtype=np.float64) + self.gamma / n
            self._heat = lambda B: np.linalg.solve(A, B)
            self._poisson = lambda B: np.linalg.solve(P, B)
        else:
            self._heat = _SparseSPD(A_heat, dtype).solve
            if n <= DENSE_LIMIT:
                P = np.asarray(negL.todense()).astype(dtype) + self.gamma / dtype(n)
                W = band_cholesky(band_from_dense(P))
                self._poisson = lambda B: band_solve(W, B)
            else:
                self.grounded = True
                g = sparse.csr_matrix(([1.0], ([n - 1], [n - 1])), shape=(n, n))
                # (the ground value enters in float64: any positive value gives the same y in exact arithmetic)
                grounded = _SparseSPD(negL + float(self.gamma) * g, dtype).solve

                def poisson(B):
                    w = grounded(B)
                    return w - w.sum(axis=0) / dtype(n)
                self._poisson = poisson

    def fields(self, sources):
        dt, n = self.dtype, self.n
        src = np.asarray(sources, dtype=np.int64)
        E = np.zeros((n, src.shape[0]), dtype=dt)
        E[src, np.arange(src.shape[0])] = 1
        u = self._heat(E)
        g = _csr_times(self.G, u, dt)
        g3 = g.reshape(-1, 3, g.shape[1])
        X = (-g3 / np.sqrt((g3 * g3).sum(axis=1, keepdims=True))).reshape(g.shape)
        b = _csr_times(self.D, X, dt)
        b = b - b.sum(axis=0) / dt(n)
        y = self._poisson(b)
        return np.ascontiguousarray((y.max(axis=0) - y).T)


def condition_numbers(A_heat, L, want_heat=True):
    """(2-norm condition number of A_heat (None unless wanted), of -L on the mean-free space), float64, from the dense operators"""
    kh = None
    if want_heat:
        eh = np.linalg.eigvalsh(np.asarray(A_heat.todense()))
        kh = float(eh[-1] / eh[0])
    el = np.linalg.eigvalsh(np.asarray((-L).todense()))      # ascending: el[0] ~ 0 belongs to the constants
    return kh, float(el[-1] / el[1])


def support_weights(phi, v0, n_loc, dmin, dmax, dtype=np.float64):
    """s = 1 - (clip(phi[v0 : v0 + n_loc], dmin, dmax) - dmin) / (dmax - dmin), the operations of k_support_weights in dtype"""
    p = np.asarray(phi, dtype=dtype)[v0:v0 + n_loc]
    dmin, dmax = dtype(dmin), dtype(dmax)
    p = np.minimum(np.maximum(p, dmin), dmax)
    return dtype(1) - (p - dmin) / (dmax - dmin)


def slab_gemm(A, Z, out, alpha, beta, nct, dtype=LD):
    """out (M x 64) with columns < 16 nct replaced by beta out + alpha A Z (beta = 0: out is not read), the others as they
    are; nct clamped to 1 .. 4.  A (M x Kc), Z (Kc x 64).  Returns a new array in dtype."""
    nct = min(max(int(nct), 1), 4)
    A, Z = np.asarray(A, dtype=dtype), np.asarray(Z, dtype=dtype)
    res = np.array(out, dtype=dtype)
    w = 16 * nct
    prod = dtype(alpha) * (A @ Z[:, :w])
    res[:, :w] = prod if beta == 0 else dtype(beta) * res[:, :w] + prod
    return res


_REF = {}


def reference(name):
    """For a named case of tests/geodesic_cases.py, computed once and shared (read-only) by the tests: dict(src = the distinct
    ids of the 64-source batch, row = id -> row, hi / lo = their fields by the longdouble / float64 model, kappa_poisson,
    kappa_heat (below 512 vertices, where the sparse mode solves the heat step by PCG too; None above), kappa = the larger)."""
    if name not in _REF:
        import geodesic_cases as gc
        ops = gc.operators(name)
        src = np.unique(gc.sources(ops[0].shape[0], 64))
        hi = HeatModel(*ops, dtype=LD).fields(src)
        lo = HeatModel(*ops, dtype=np.float64).fields(src)
        kh, kp = condition_numbers(ops[0], ops[1], want_heat=ops[0].shape[0] < 512)
        for a in (hi, lo):
            a.setflags(write=False)
        _REF[name] = dict(src=src, row={int(s): q for q, s in enumerate(src)}, hi=hi, lo=lo, kappa_heat=kh, kappa_poisson=kp,
                          kappa=max(kp, kh) if kh is not None else kp)
    return _REF[name]


def rows(ref, which, ids):
    """the model fields (which = "hi" / "lo") of the source ids, in their order"""
    return ref[which][[ref["row"][int(s)] for s in ids]]
