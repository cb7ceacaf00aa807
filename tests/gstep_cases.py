"""Shared by tests/test_gpu_gstep.py: the fixtures of tools/gen_golden_gstep.py, a stiffer synthetic case, the longdouble
model of the product kernel and the bounds the file holds the global step to.

Product kernel.  out[f, m, d] = sum_n rhs[f, n, d] Ainv[n, m] is an N-term chain of FMAs (in groups of four inside an MFMA), so
against the exact sum of the SAME operands -- the device's own inverse, downloaded -- an entry is within

    (N + 4) eps sum_n |rhs[f, n, d]| |Ainv[n, m]|

(gamma_N <= N eps (1 + N eps); the + 4 covers the zero-padded terms of the last stage).

Global step.  q = A^-1 (b + M / h^2 s) against the reference's sparse factorisation:

    |q_dev - q_ref|  <=  || |A^-1| ||_inf  max (force bound)  +  64 eps kappa(A) max |q_ref|

  * first term: the device's b differs from the reference's by the bound tests/test_gpu_cforces.py derives for the fixture
    (per vertex; its maximum here), and A^-1 passes an entrywise error on with its absolute row sums.
  * second term: both solves are backward stable -- the explicit inverse of an SPD matrix applied to a vector, and the LU
    of the reference -- so each is within a small multiple of eps kappa(A) |q| of the exact solution; 64 is the margin the
    set-up test below holds the inverse itself to.  The inertia term M / h^2 s is formed with three roundings per entry on both
    sides, (a few) eps M / h^2 |s|; A^-1 M / h^2 has entries below 1 in absolute row sum times kappa, so this lies inside
    the same term.
kappa(A): NumPy's 2-norm condition number of the dense matrix."""
import numpy as np
from scipy import sparse

from conftest import load_golden

EPS = np.finfo(np.float64).eps
KINDS = ["edge_spring", "tris_strain", "tets_strain", "tets_deformation_gradient"]
_cache = {}


def golden(name):
    """The gstep fixture ``name`` (a kind or "combined"), read once and read-only, with ``A`` (dense), ``Ainv_abs_inf`` =
    || |A^-1| ||_inf and ``kappa``."""
    if name not in _cache:
        z = load_golden("gstep_" + name)
        for v in z.values():
            v.setflags(write=False)
        A = sparse.coo_matrix((z["val"], (z["row"], z["col"])), shape=tuple(z["shape"])).toarray()
        z["A"] = A
        z["Ainv_abs_inf"] = np.abs(np.linalg.inv(A)).sum(axis=1).max()
        z["kappa"] = np.linalg.cond(A)
        assert abs(z["kappa"] - float(z["cond"])) <= 1e-9 * z["kappa"]
        _cache[name] = z
    return _cache[name]


def step_bound(z, force_bound):
    """Per velocity mode the scalar bound of the module docstring."""
    return {mode: z["Ainv_abs_inf"] * float(np.max(force_bound)) + 64 * EPS * z["kappa"] * np.abs(z["q_" + mode]).max()
            for mode in ("zero", "difference")}


def product_model(rhs, Ainv):
    """(exact-ish sum in longdouble, sum of absolute values) of out[f, m, d] = sum_n rhs[f, n, d] Ainv[n, m]."""
    R, B = rhs.astype(np.longdouble), Ainv.astype(np.longdouble)
    out = np.einsum("fnd,nm->fmd", R, B)
    mag = np.einsum("fnd,nm->fmd", np.abs(R), np.abs(B))
    return out, mag.astype(np.float64)


def spd_band(n, rng):
    """A symmetric, strictly diagonally dominant band matrix (CSR, sorted): positive definite, entries of mixed size."""
    A = sparse.lil_matrix((n, n))
    for k in (1, 3):
        for i in range(n - k):
            v = -rng.uniform(0.1, 1.0)
            A[i, i + k] = v
            A[i + k, i] = v
    A = A.tocsr()
    d = np.asarray(abs(A).sum(axis=1)).ravel() + rng.uniform(0.05, 2.0, size=n)
    A = (A + sparse.diags(d)).tocsr()
    A.sort_indices()
    return A


def box_tets(nx, ny, nz, h):
    """nx x ny x nz vertices, every cell split into the six tetrahedra along its main diagonal."""
    vid = lambda i, j, k: (i * ny + j) * nz + k
    V = np.array([[i * h, j * h, k * h] for i in range(nx) for j in range(ny) for k in range(nz)], dtype=np.float64)
    T = []
    perms = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
    for i in range(nx - 1):
        for j in range(ny - 1):
            for k in range(nz - 1):
                for pm in perms:
                    c = [i, j, k]
                    tet = [vid(*c)]
                    for a in pm:
                        c[a] += 1
                        tet.append(vid(*c))
                    T.append(tet)
    return V, np.array(T, dtype=np.int64)


def stiff_case():
    """A 5 x 5 x 4 grid of tetrahedra (N = 100: four vertex tiles of the product kernel, the last partial) with wi = 1e3,
    h = 0.1 and masses spread over a factor of six: stiff enough for the inverse to lose digits, kappa in 1e2 .. 1e6."""
    if "stiff" not in _cache:
        from animsnapbases_amd import projections as proj
        rest, tets = box_tets(5, 5, 4, 0.5)
        N = rest.shape[0]
        assert N == 100
        masses = 0.02 * (1.0 + 5.0 * np.random.default_rng(11).random(N))
        wi, dt = 1e3, 0.1
        A = proj.global_matrix([(proj.build_setup("tets_strain", tets, rest), wi)], N, masses, dt)
        kappa = np.linalg.cond(A.toarray())
        assert 1e2 <= kappa <= 1e6, kappa
        _cache["stiff"] = dict(rest=rest, tets=tets, masses=masses, wi=wi, dt=dt, A=A, kappa=kappa)
    return _cache["stiff"]
