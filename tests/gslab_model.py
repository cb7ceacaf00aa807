"""Shared by tests/test_gslab_cpu.py and tests/test_gpu_gslab.py: a NumPy f64 model of the global step's block-tridiagonal slab
solver (csrc/asb_gslab.hip), the longdouble-refined host solution it and the device are compared with, and the matrices of the
sweep tests.

The model is the two-product scheme of the device, in its order:

    set-up     S_0 = A_00,  S_k = A_kk - (C_k S_{k-1}^-1) C_k^T,  C_k = A_{k,k-1} sparse;  only S_k^-1 is kept, padded to a multiple
               of 16 by an identity block
    forward    u_k = S_k^-1 (b_k - C_k u_{k-1})
    backward   x_k = u_k - S_k^-1 (C_{k+1}^T x_{k+1})

Reference.  ``refined_solve``: SciPy's ``splu`` followed by iterative refinement with the residual b - A x formed in
numpy.longdouble (the x87 format here: 64-bit mantissa), until the correction falls below a longdouble epsilon of the solution
or stalls: what remains of the error is eps_ld kappa(A), 2^-11 of what a float64 solve can reach.

Bound.  The form of DESIGN.md 3.13 for a backward-stable solve with an explicit inverse: 64 eps kappa(A) max |x|, kappa the 2-norm
condition number of the dense matrix (``numpy.linalg.cond``; for the chain of 50 001 vertices, where the dense matrix is not
formed, the Gershgorin bound max_i sum_j |a_ij| / min_i (a_ii - sum_{j != i} |a_ij|) >= kappa, finite because the mass term makes A
strictly diagonally dominant).  Nothing is fitted."""
import numpy as np
from scipy import sparse
from scipy.sparse.linalg import splu

EPS = np.finfo(np.float64).eps
LD = np.longdouble
_cache = {}


def _pad16(n):
    return (n + 15) // 16 * 16


def slab_factor(A_perm, slab_ptr):
    """The model's factor of the permuted CSR: per slab (S_k^-1 padded (sp, sp), C_k CSR (n_k, n_{k-1}) or None)."""
    ptr = [int(p) for p in slab_ptr]
    A = sparse.csr_matrix(A_perm)
    fac, prev = [], None
    for k in range(len(ptr) - 1):
        a, b = ptr[k], ptr[k + 1]
        S = A[a:b, a:b].toarray()
        C = None
        if k > 0:
            C = A[a:b, ptr[k - 1]:a].tocsr()
            Ct = A[ptr[k - 1]:a, a:b].toarray()                    # C_k^T as the device takes it: from the rows of slab k - 1
            S = S - (C @ prev[:a - ptr[k - 1], :a - ptr[k - 1]]) @ Ct
        sp = _pad16(b - a)
        Sp = np.eye(sp)
        Sp[:b - a, :b - a] = S
        Si = np.linalg.inv(Sp)
        Si = 0.5 * (Si + Si.T)
        fac.append((Si, C))
        prev = Si
    return fac


def slab_solve(fac, slab_ptr, B):
    """x = A^-1 B (permuted numbering, B (N, w)) by the forward and the backward sweep."""
    ptr = [int(p) for p in slab_ptr]
    ns = len(ptr) - 1
    X = np.array(B, dtype=np.float64)
    for k in range(ns):
        a, b = ptr[k], ptr[k + 1]
        t = X[a:b] if k == 0 else X[a:b] - fac[k][1] @ X[ptr[k - 1]:a]
        X[a:b] = fac[k][0][:b - a, :b - a] @ t
    for k in range(ns - 2, -1, -1):
        a, b = ptr[k], ptr[k + 1]
        t = fac[k + 1][1].T @ X[b:ptr[k + 2]]
        X[a:b] = X[a:b] - fac[k][0][:b - a, :b - a] @ t
    return X


def model_solve(A, plan, B):
    """A^-1 B in the ORIGINAL numbering through the model, for a plan of ``projections.slab_plan``."""
    X = slab_solve(slab_factor(plan.A_perm, plan.slab_ptr), plan.slab_ptr, np.asarray(B)[plan.order])
    out = np.empty_like(X)
    out[plan.order] = X
    return out


def refined_solve(A, B, sweeps=8):
    """The longdouble-refined solution of A X = B as float64-pairs collapsed to longdouble (N, w)."""
    A = sparse.csc_matrix(A)
    lu = splu(A)
    Al = sparse.csr_matrix(A).astype(LD)
    Bl = np.asarray(B, dtype=LD)
    X = lu.solve(np.asarray(B, dtype=np.float64)).astype(LD)
    last = np.inf
    for _ in range(sweeps):
        R = Bl - Al @ X
        d = lu.solve(np.asarray(R, dtype=np.float64)).astype(LD)
        X = X + d
        size = float(np.abs(d).max())
        if size <= float(np.finfo(LD).eps) * float(np.abs(X).max()) or size >= last:
            break
        last = size
    return X


def gershgorin_kappa(A):
    """An upper bound of kappa_2(A) for a strictly diagonally dominant symmetric A."""
    A = sparse.csr_matrix(A)
    d = A.diagonal()
    off = np.asarray(abs(A).sum(axis=1)).ravel() - np.abs(d)
    assert (d - off > 0).all()
    return float((d + off).max() / (d - off).min())


def bound(kappa, X):
    return 64.0 * EPS * kappa * float(np.abs(np.asarray(X, dtype=np.float64)).max())


# ------------------------------------------------------------------ the matrices of the sweep tests
def chain_matrix(n, seed=0):
    """The system matrix of an edge-spring chain of n vertices (wi = 2, dt = 0.25; n = 1: the mass term alone), its numbering
    scattered by a fixed permutation so that the plan has work to do."""
    from animsnapbases_amd import projections as proj
    from pdsolve_cases import chain
    rest, edges, m = chain(max(n, 2))
    rest, m = rest[:n], m[:n]
    if n == 1:
        return sparse.csr_matrix(np.array([[m[0] / 0.25 ** 2]]))
    perm = np.random.default_rng(77 + n + seed).permutation(n)
    A = proj.global_matrix([(proj.build_setup("edge_spring", perm[edges], rest[np.argsort(perm)]), 2.0)], n, m, 0.25)
    return A


def grid_matrix(nx, wi, m0=0.3, seed=3, dt=0.1):
    """The tets_strain matrix of an nx^3 grid of vertices (six tetrahedra per cell, ``gstep_cases.box_tets``) in a scattered
    numbering, masses m0 .. 6 m0.  10^3, wi = 1e3, m0 = 0.3: kappa = 57.5; 8^3, wi = 1e6, m0 = 0.02: kappa = 8.5e5."""
    from animsnapbases_amd import projections as proj
    from gstep_cases import box_tets
    key = ("grid", nx, wi, m0, seed, dt)
    if key not in _cache:
        rest, tets = box_tets(nx, nx, nx, 0.5)
        N = rest.shape[0]
        rng = np.random.default_rng(seed)
        perm = rng.permutation(N)
        masses = m0 * (1.0 + 5.0 * rng.random(N))
        A = proj.global_matrix([(proj.build_setup("tets_strain", perm[tets], rest[np.argsort(perm)]), wi)], N, masses, dt)
        _cache[key] = A
    return _cache[key]


def rhs(n, w, seed):
    """(n, w) right-hand sides of mixed size."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, w)) * 10.0 ** rng.integers(-2, 3, size=(n, 1))
