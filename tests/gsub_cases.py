"""Shared by tests/test_gsub_cpu.py and tests/test_gpu_gsub.py: the cases of the global step in a position subspace and the
bounds its device results are held to.  Nothing is fitted to the code under test; every term is derived here.

ONE APPLICATION.  The device computes Y = W R and Q = o' + U Y with W = fl(U At^-1)^T, At = U^T A U inverted by the dense layer.
  chains    Two dot-product chains, of length N (Y) and r (Q), and a third of length r inside W = U At^-1; each entry of a chain
            of length n carries at most (n + c) eps times the sum of the absolute values of its terms.  All three sums are
            entries of |U| (|At^-1| (|U^T| |R|)) (``Galerkin.magnitude``), hence (N + 2 r + 16) eps max of that matrix.
  inverse   At^-1 itself: the form of DESIGN.md 3.13 for an explicit inverse, 64 eps kappa(At_d) max |x|, with x the largest
            entry of |U| |z|, z = At^-1 U^T R the coefficients the inverse's error multiplies (``Galerkin.coefficients``; it is
            at least max |P R|).
  origin    (affine only) o' = o - P A o: the two terms above for R = A o, the sparse product A o -- (row entries + 2) eps |A| |o|
            passed through |U| |At^-1| |U^T| -- the subtraction's 2 eps max |o|, and the final add's eps max |q|.

K ITERATIONS of the public path.  One iteration commits the error of the right-hand side passed through P -- || |P| ||_inf
(``p_abs_inf``) times the force bound of the existing tests -- plus one application; K iterations are held to
``pdsolve_cases.bound_K(one, K, amp)`` with amp MEASURED ON THE HOST MODEL under the subspace solver
(``pdsolve_cases.measure_amp`` on the case whose ``lu`` is the ``Galerkin`` object).

The cases: origin = frame 0 and, per coordinate, the leading right singular vectors of frames - frame 0 of the five pdsolve
fixtures (N = 18 and 42, 130 frames, kappa(A) <= 4.5).  Checked on the host (tests/test_gsub_cpu.py): frames - frame 0 has full
rank N in every coordinate; amp stays below 8 for r in {4, 8, N} at K in {1, 3, 10}, far below AMP_CAP = 1000, so no frame and no
case is left out; the r = N model equals the full model to 4e-15; the r in {4, 8} models differ from it by 0.058 .. 1.3."""
import numpy as np

import pdsolve_cases as pc
from gsub_model import EPS, Galerkin, svd_basis, vertex_major

RANKS = (4, 8)
_cache = {}


def apply_bound(g, R, affine=True, result_max=None):
    """The bound of one application (module docstring) for the right-hand side ``R`` (3 N, w), as one number."""
    R = np.asarray(R, dtype=np.float64)
    chains = (g.N + 2 * g.r + 16) * EPS * float(g.magnitude(R).max())
    co = g.coefficients(R)
    inverse = 64 * EPS * max(g.kappa[d] * float(co[d::3].max()) for d in range(3))
    total = chains + inverse
    if affine:
        Ao = vertex_major(np.asarray(g.Ao, dtype=np.float64)[None])
        A64, o64 = np.abs(g.A).astype(np.float64), np.abs(g.o).astype(np.float64)
        row = int((A64 != 0).sum(axis=1).max())
        sparse_err = (row + 2) * EPS * float(g.magnitude(vertex_major((A64 @ o64)[None])).max())
        qmax = float(np.abs(g.apply(R, True)).max()) if result_max is None else float(result_max)
        total += apply_bound(g, Ao, False) + sparse_err + 2 * EPS * float(o64.max()) + EPS * qmax
    return total


def residual_bound(g, one):
    """|U_d^T (A q - rhs)| of a result within ``one`` of the exact Galerkin step (whose residual is zero): || |U^T| |A| ||_inf one."""
    return max(float((np.abs(g.U[d].T) @ np.abs(g.A)).astype(np.float64).sum(axis=1).max()) for d in range(3)) * one


def setup_residual_bound(g):
    """What the set-up reports, max_d max |U_d^T (A x_d - 1)| with x_d = P_d 1 from the device: the residual bound of that
    application, plus the sparse product A x ((row entries + 2) eps |A| |x|), the subtraction and the chain of length N over
    |U^T| |A x - 1| <= |U^T| (|A| |x| + 1)."""
    ones = np.ones((3 * g.N, 1))
    x = np.abs(g.apply(ones, False)).astype(np.float64)
    A64 = np.abs(g.A).astype(np.float64)
    row = int((A64 != 0).sum(axis=1).max())
    size = max(float((np.abs(g.U[d].T).astype(np.float64) @ (A64 @ x[d::3] + 1.0)).max()) for d in range(3))
    return residual_bound(g, apply_bound(g, ones, False)) + (g.N + row + 12) * EPS * size


def p_abs_inf(g):
    return max(float(np.abs(g.P(d)).astype(np.float64).sum(axis=1).max()) for d in range(3))


def sub_case(name, r=None, load=pc._load, base=None):
    """The host case of ``pdsolve_cases.host_case(name)`` (or ``base``, a case shaped like it) with its ``lu`` replaced by the
    Galerkin map of the fixtures' basis (r components, None: all N): also ``comps`` (K, N, 3), ``Qt``, ``origin``, ``galerkin``."""
    key = (name, r)
    if base is not None or key not in _cache:
        from animsnapbases_amd import projections as proj
        c = pc.host_case(name, load) if base is None else base
        comps = svd_basis(c["frames"])
        Qt = proj.subspace_basis(comps, r)
        g = Galerkin(c["A"], Qt, c["frames"][0])
        out = dict(c, lu=g, galerkin=g, comps=comps, Qt=Qt, origin=np.array(c["frames"][0]), r=Qt.shape[1])
        if base is not None:
            return out
        _cache[key] = out
    return _cache[key]


def rhs_of(c, q, s, reduced=None, extra=None):
    """The right-hand side of the iteration that starts at ``q`` (F', N, 3): sum of the kinds' terms + M / dt^2 s (+ ``extra``)."""
    from animsnapbases_amd import projections as proj
    b = (c["masses"] / c["dt"] ** 2)[None, :, None] * s
    if extra is not None:
        b = b + extra
    for i, (setup, St, smin, smax) in enumerate(c["kinds"]):
        if reduced is not None and reduced[0] == i:
            b = b + pc.reduced_term(setup, St, reduced[1], q, smin, smax)
        else:
            p = proj.project_host(setup, q, smin, smax)
            b = b + np.stack([St @ p[f] for f in range(q.shape[0])])
    return b


def amps(c, mode, Ks=pc.KS, reduced=None):
    """``pdsolve_cases.measure_amp`` on the subspace case, cached per (fixture, r, mode, reduced kind)."""
    key = ("amp", c["name"], c["r"], mode, None if reduced is None else (reduced[0], id(reduced[1])))
    if key not in _cache:
        _cache[key] = pc.measure_amp(c, mode, Ks, reduced=reduced)
    return _cache[key]


def hyper_bound(g, ms, M, coef, result_max):
    """One application on the hyper-reduced path, where the device forms c = o' + P ms and G = P M apart and adds G coef: the
    bound of the affine map on ms, plus per coordinate the two terms of the linear map on the columns of M (3, N, mp) weighted
    by |coef| (3, mp, F') -- chains: (N + 2 r + 16) eps max (magnitude(M) |coef|); inverse: 64 eps kappa sum_j max(|U| |z_j|)
    max_f |coef_j|."""
    total = apply_bound(g, vertex_major(ms), True, result_max)
    Mv = np.ascontiguousarray(np.asarray(M).transpose(1, 0, 2).reshape(3 * g.N, -1))       # row 3 v + d: M_d[v, :]
    mag, co = g.magnitude(Mv), g.coefficients(Mv)
    for d in range(3):
        a = np.abs(coef[d])
        total += (g.N + 2 * g.r + 16) * EPS * float((mag[d::3] @ a).max())
        total += 64 * EPS * g.kappa[d] * float((co[d::3].max(axis=0) * a.max(axis=1)).sum())
    return total
