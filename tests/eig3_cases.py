"""Symmetric 3 x 3 test matrices for the two eigen-solvers of csrc/asb_kernels.h (eig3_top, eig3_top_fast), their 60-digit
reference (mpmath) and the per-matrix error measures shared by tests/test_deflate_step_cpu.py (host) and
tests/test_gpu_deflate_step.py (device).  Not a test module.

A matrix travels as a6 = (a00, a01, a02, a11, a12, a22), a result as out4 = (lambda, u0, u1, u2).

Error measures are normalised so that one literal per family serves every scale:
    lam  = |lambda - lambda_ref|            / (eps max|a_ij|)
    res  = max |A u - lambda u|             / (eps max|a_ij|)        (evaluated in mpmath)
    ang  = sin(angle(u, u_ref)) gap_ref     / (eps max|a_ij|)        only where gap_ref = lambda_1 - lambda_2 >= 1e-3 lambda_1
    sub  = |u - P u| gap_out                / (eps max|a_ij|)        elsewhere: P projects on the eigenvectors of the cluster
                                                                     { lambda_i > lambda_1 (1 - 1e-3) }, gap_out = lambda_1 - the
                                                                     largest eigenvalue outside it (cluster = all three: every
                                                                     unit vector is a top eigenvector, nothing to measure)
"""
import itertools

import mpmath as mp
import numpy as np

EPS = 2.0 ** -52
DPS = 60
SCALES = (1e-240, 1e-150, 1.0, 1e150, 1e240)
NEAR_LIMIT = 9.9e299            # largest entry of the last scaled case: just under the solvers' `sc < 1e300` switch
REL_GAPS = (0.0, 1e-3, 1e-6, 1e-7, 1e-9, 1e-12, 1e-15)

# Tolerances.  The reference's own solver for this step is LAPACK, so the bar is LAPACK's error on the same matrices
# (numpy.linalg.eigh, f64, against the same 60-digit reference; measured once, figures in tests/README.md): per family 8 x LAPACK's
# worst normalised error, never below 16 (the textbook bound of a backward-stable 3 x 3 solve, so that a family where LAPACK
# happens to be exact does not make the bar zero).  family -> LAPACK's worst (lam, res, ang, sub), literals rounded up to three
# digits; tests/test_deflate_step_cpu.py::test_lapack_error_is_what_the_bars_were_derived_from measures them again:
LAPACK_WORST = {
    "gram": (4.09, 4.09, 2.41, 0.0),
    "rank12": (5.29, 5.84, 5.34, 0.0),
    "double": (4.0, 2.95, 0.943, 1.58),
    "near_identity": (3.37, 3.15, 1.86, 1.25),
    "diagonal": (0.8, 0.8, 0.0, 0.0),
}
MARGIN, FLOOR = 8.0, 16.0
UNIT_TOL = 4 * EPS


def bounds(family):
    return dict(zip(("lam", "res", "ang", "sub"), (max(MARGIN * w, FLOOR) for w in LAPACK_WORST[family])))


def a6_of(G):
    G = np.asarray(G, dtype=np.float64)
    return np.array([G[0, 0], G[0, 1], G[0, 2], G[1, 1], G[1, 2], G[2, 2]])


def mat_of(a6):
    a = [float(x) for x in a6]
    return [[a[0], a[1], a[2]], [a[1], a[3], a[4]], [a[2], a[4], a[5]]]


def _rand_orth(rng):
    Q, R = np.linalg.qr(rng.normal(size=(3, 3)))
    return Q * np.sign(np.diag(R))


def base_families():
    """name -> list of a6 (float64), at their natural scale."""
    rng = np.random.default_rng(20240531)
    fam = {}
    # random Gram matrices of 3 x F slabs, row scales over 1e-3 .. 1e3
    g = []
    for i in range(48):
        F = int(rng.integers(3, 200))
        S = rng.normal(size=(3, F)) * 10.0 ** rng.uniform(-3, 3, size=(3, 1))
        g.append(a6_of(S @ S.T))
    fam["gram"] = g
    # rank 1 and rank 2 exactly: integer slabs, Gram matrices formed in integers
    r = []
    for i in range(12):
        a, b = rng.integers(-9, 10, size=3), rng.integers(-9, 10, size=17)
        if not a.any():
            a[i % 3] = 1
        if not b.any():
            b[0] = 1
        S = np.outer(a, b)
        r.append(a6_of((S @ S.T).astype(np.float64)))
    for a in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, -1, 1], [3, 4, 0]):      # motion along an axis / a diagonal
        S = np.outer(np.array(a), np.arange(1, 12))
        r.append(a6_of((S @ S.T).astype(np.float64)))
    for i in range(12):
        S = np.outer(rng.integers(-9, 10, size=3), rng.integers(-9, 10, size=17)) + \
            np.outer(rng.integers(-9, 10, size=3), rng.integers(-9, 10, size=17))
        r.append(a6_of((S @ S.T).astype(np.float64)))
    fam["rank12"] = r
    # top two eigenvalues equal exactly (lambda I - c m m^T, integers) and apart by REL_GAPS (rotated diag(1, 1 - d, mu))
    d = []
    for m, lam, c in (([1, 2, 2], 20, 1), ([1, 0, 0], 7, 3), ([0, 1, 0], 7, 7), ([0, 0, 1], 5, 2), ([1, 1, 1], 12, 2), ([3, -1, 2], 100, 5)):
        m = np.array(m, dtype=np.float64)
        d.append(a6_of(lam * np.eye(3) - c * np.outer(m, m)))
    # motion on a circle: the slab (cos, sin, 0) r over a whole period has a double top singular value up to rounding
    t = 2 * np.pi * np.arange(64) / 64
    for Q in (np.eye(3), _rand_orth(rng)):
        S = Q @ np.stack([np.cos(t), np.sin(t), 0.25 * np.cos(3 * t)])
        d.append(a6_of(S @ S.T))
    for gap in REL_GAPS:
        for mu in (0.0, 0.3, 0.999):
            for rep in range(2):
                Q = _rand_orth(rng)
                d.append(a6_of((Q * np.array([1.0, 1.0 - gap, mu * (1.0 - gap)])) @ Q.T))
    fam["double"] = d
    # all three equal, and lambda I + t E down to t = 1e-17 lambda
    n = [a6_of(lam * np.eye(3)) for lam in (1.0, 3.0, 0.1, 1e-5, 12345.678)]
    for tt in (1e-1, 1e-3, 1e-6, 1e-8, 1e-10, 1e-12, 1e-14, 1e-15, 1e-16, 1e-17):
        for lam in (1.0, 0.7, 1234.5):
            E = rng.uniform(-1, 1, size=(3, 3))
            E = (E + E.T) / 2
            n.append(a6_of(lam * (np.eye(3) + tt * E)))
    fam["near_identity"] = n
    # diagonal matrices in all six orders of their entries (distinct, two equal, one zero, far apart)
    g = []
    for trip in ((3.0, 2.0, 1.0), (5.0, 5.0, 1.0), (5.0, 1.0, 1.0), (2.0, 1.0, 0.0), (1.0, 1e-8, 1e-16), (1.0, 1.0 - 2.0 ** -52, 0.5)):
        for perm in sorted(set(itertools.permutations(trip))):
            g.append(a6_of(np.diag(perm)))
    fam["diagonal"] = g
    return fam


def all_cases():
    """list of (family, label, a6): every base matrix at SCALES and with its largest entry at NEAR_LIMIT; the zero matrix once."""
    out = []
    for name, mats in base_families().items():
        for i, a in enumerate(mats):
            sc = np.abs(a).max()
            for s in SCALES:
                out.append((name, "%s[%d]*%g" % (name, i, s), a * s))
            out.append((name, "%s[%d]->%g" % (name, i, NEAR_LIMIT), a * (NEAR_LIMIT / sc)))
    out.append(("zero", "zero", np.zeros(6)))
    return out


def reference(a6):
    """60-digit eigen-decomposition: lam (descending, mpf), vecs (matching unit vectors as lists of mpf), sc = max|a_ij| (float)."""
    with mp.workdps(DPS):
        A = mp.matrix(mat_of(a6))
        E, Q = mp.eigsy(A)
        order = sorted(range(3), key=lambda i: E[i], reverse=True)
        lam = [E[i] for i in order]
        vecs = []
        for i in order:
            v = [Q[r, i] for r in range(3)]
            nv = mp.sqrt(sum(x * x for x in v))
            vecs.append([x / nv for x in v])
    return dict(lam=lam, vecs=vecs, sc=float(np.abs(np.asarray(a6, dtype=np.float64)).max()))


def sign_skipped(ref):
    """the canonical-sign check is skipped where the two largest magnitudes of u_ref are within 1e-8 of each other"""
    m = sorted((abs(float(x)) for x in ref["vecs"][0]), reverse=True)
    return m[0] - m[1] <= 1e-8


def cluster_of(ref):
    """indices of the eigenvalues that count as the (nearly) multiple top eigenvalue"""
    l1 = ref["lam"][0]
    return [i for i in range(3) if i == 0 or ref["lam"][i] > l1 * (1 - mp.mpf("1e-3"))]


def measure(a6, out4, ref):
    """dict of the normalised error measures of the module's docstring (None where one does not apply), plus `finite`, `unit`
    (| |u| - 1 |, absolute) and `sign_ok`."""
    out4 = np.asarray(out4, dtype=np.float64)
    res = dict(finite=bool(np.isfinite(out4).all()), lam=None, res=None, ang=None, sub=None, unit=None, sign_ok=None)
    if not res["finite"]:
        return res
    u = out4[1:]
    res["sign_ok"] = bool(u.max() == np.abs(u).max())
    sc = ref["sc"]
    with mp.workdps(DPS):
        A = mp.matrix(mat_of(a6))
        um = [mp.mpf(float(x)) for x in u]
        lm = mp.mpf(float(out4[0]))
        res["unit"] = float(abs(mp.sqrt(sum(x * x for x in um)) - 1))
        lam_err = abs(lm - ref["lam"][0])
        r = max(abs(sum(A[i, j] * um[j] for j in range(3)) - lm * um[i]) for i in range(3))
        if sc == 0.0:
            res["lam"], res["res"] = float(lam_err), float(r)          # must be exactly zero
            return res
        unit = EPS * mp.mpf(sc)
        res["lam"], res["res"] = float(lam_err / unit), float(r / unit)
        cl = cluster_of(ref)
        # component of u outside the span of the cluster's eigenvectors
        d = list(um)
        for i in cl:
            v = ref["vecs"][i]
            c = sum(a * b for a, b in zip(um, v))
            d = [a - c * b for a, b in zip(d, v)]
        dn = mp.sqrt(sum(x * x for x in d))
        if len(cl) == 1:
            res["ang"] = float(dn * (ref["lam"][0] - ref["lam"][1]) / unit)
        elif len(cl) == 2:
            res["sub"] = float(dn * (ref["lam"][0] - ref["lam"][2]) / unit)
    return res


def lapack(a6):
    """LAPACK (numpy.linalg.eigh, f64) on the same matrix, as out4"""
    w, V = np.linalg.eigh(np.array(mat_of(a6)))
    return np.array([w[-1], V[0, -1], V[1, -1], V[2, -1]])


def check_case(family, label, a6, out4, ref, who):
    """every per-matrix demand on a solver's result; returns the measures"""
    m = measure(a6, out4, ref)
    assert m["finite"], "%s %s: %r" % (who, label, out4)
    assert m["unit"] <= UNIT_TOL, "%s %s: | |u| - 1 | = %.3g" % (who, label, m["unit"])
    if not sign_skipped(ref):
        assert m["sign_ok"], "%s %s: sign of u = %r" % (who, label, out4[1:])
    if family == "zero":
        assert out4[0] == 0.0 and m["res"] == 0.0, "%s %s: %r" % (who, label, out4)
        return m
    b = bounds(family)
    for key in ("lam", "res", "ang", "sub"):
        if m[key] is not None:
            assert m[key] <= b[key], "%s %s: %s = %.4g x eps max|a| (bound %.4g)" % (who, label, key, m[key], b[key])
    return m
