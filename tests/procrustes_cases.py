"""3 x 3 cross-covariance matrices for the rotation solve of snapshot ingest (procrustes_rot, csrc/asb_kernels.h), their
60-digit reference (mpmath SVD of the STORED matrix) and the error measures shared by tests/test_procrustes_rot_cpu.py (host
probe) and tests/test_gpu_procrustes.py (the 3 x 3 part of the bound on T).  Not a test module.

A matrix M is built from chosen factors U diag(s) V^T (or as an exact integer product for the deficient families), rounded once to
float64 and scaled; the expected R is computed from what was stored, never from the chosen factors:
    full rank   R_ref = U V^T, times -1 where its determinant is negative (utils/process.py:223-227 of the reference)
    rank 2      R_ref = U diag(1, 1, det U det V) V^T: the proper rotation, which is the reference's result whenever LAPACK's free
                sign of u3 / v3 comes out positive
    rank 1      no unique R: finite, orthogonal, proper, and optimal  tr(R^T M) >= s1 (1 - b eps)
    rank 0      the identity exactly
Which rule applies is decided by the reference alone (`kind_of`): s3 / s1 >= 1e-10 is full rank, <= 1e-15 deficient, and no case
may lie between (the band the solver's own threshold decides).

Error measures, normalised so that one literal per family serves every scale (eps = 2^-52):
    rot   = max |R - R_ref| (s2 + s3) / (eps s1)       s1 / (s2 + s3) is the conditioning of the polar factor
    orth  = max |R^T R - I| / eps                      evaluated in mpmath
    det   = |det R - 1| / eps                          rank 1 only
    opt   = max(0, s1 - tr(R^T M)) / (eps s1)          rank 1 only
"""
import itertools

import mpmath as mp
import numpy as np

EPS = 2.0 ** -52
DPS = 60
SCALES = (1e-150, 1e-8, 1.0, 1e8, 1e150)
FULL_MIN = 1e-10            # s3 / s1 of every full-rank case is at least this
DEFICIENT_MAX = 1e-15       # the first negligible singular value of a deficient case is at most this x s1
THIN = (1e-2, 1e-4, 1e-6, 1e-8, 1e-10)

# Tolerances: the reference's solver for this step is LAPACK (numpy.linalg.svd), so the bar is LAPACK's own error on the same
# matrices against the same 60-digit reference -- R = U @ Vt with the rule of the case's kind, measured once (figures in
# tests/README.md).  Per family and measure 8 x LAPACK's worst, never below 16.  family -> LAPACK's worst (rot, orth, det, opt),
# rounded up to three digits; test_procrustes_rot_cpu.py::test_lapack_error_is_what_the_bars_were_derived_from measures them again:
LAPACK_WORST = {
    "generic": (5.09, 6.7, 0.0, 0.0),
    "mirrored": (5.71, 6.68, 0.0, 0.0),
    "thin": (9.89, 8.95, 0.0, 0.0),
    "rank2": (1.68, 6.68, 0.0, 0.0),
    "rank1": (0.0, 6.58, 6.0, 2.49),
    "repeated": (35.7, 6.82, 0.0, 0.0),
    "diagonal": (0.501, 1.0, 0.0, 0.0),
}
MARGIN, FLOOR = 8.0, 16.0
MEASURES = ("rot", "orth", "det", "opt")


def bounds(family):
    return dict(zip(MEASURES, (max(MARGIN * w, FLOOR) for w in LAPACK_WORST[family])))


def _rand_orth(rng, det):
    Q, R = np.linalg.qr(rng.normal(size=(3, 3)))
    Q = Q * np.sign(np.diag(R))
    if np.linalg.det(Q) * det < 0:
        Q[:, 2] *= -1
    return Q


def _usv(rng, s, det):
    """U diag(s) V^T with det U det V = det, rounded once"""
    du = 1.0 if rng.random() < 0.5 else -1.0
    return (_rand_orth(rng, du) * np.asarray(s, dtype=np.float64)) @ _rand_orth(rng, du * det).T


def base_families():
    """name -> list of 3 x 3 float64 matrices with s1 of order 1 .. 1e3"""
    rng = np.random.default_rng(20241018)
    fam = {}
    for name, det in (("generic", 1.0), ("mirrored", -1.0)):
        g = []
        for i in range(12):
            r3 = rng.uniform(0.1, 1.0)
            g.append(_usv(rng, (1.0, rng.uniform(r3, 1.0), r3), det))
        fam[name] = g
    # s3 / s1 = 1e-2 .. 1e-10 (a hair above, so that the stored matrix stays on the full-rank side of FULL_MIN after rounding:
    # rounding M moves s3 by up to eps s1 = 2e-6 s3 there), s2 / s1 in [0.1, 1], both signs of det M
    t = []
    for r3 in THIN:
        for det in (1.0, -1.0):
            for rep in range(3):
                t.append(_usv(rng, (1.0, rng.uniform(0.1, 1.0), r3 * (1.0 + 1e-4)), det))
    fam["thin"] = t
    # rank 2 exactly: (3 x 2 integers) (2 x 3 integers), formed in integers; a flat sheet in a coordinate plane among them
    r = []
    while len(r) < 12:
        A, B = rng.integers(-9, 10, size=(3, 2)), rng.integers(-9, 10, size=(2, 3))
        if np.linalg.matrix_rank(A) == 2 and np.linalg.matrix_rank(B) == 2:
            r.append((A @ B).astype(np.float64))
    for A, B in (([[1, 0], [0, 1], [0, 0]], [[3, 1, 0], [-1, 2, 0]]), ([[2, 1], [1, 3], [0, 0]], [[1, 0, 2], [0, 1, -1]]),
                 ([[0, 0], [1, 0], [0, 1]], [[0, 5, 0], [0, 0, 5]]), ([[1, 2], [2, 1], [3, 3]], [[1, 0, 0], [0, 1, 0]])):
        r.append((np.array(A) @ np.array(B)).astype(np.float64))
    fam["rank2"] = r
    # rank 1 exactly: outer products of small integer vectors, along an axis / a diagonal among them
    r = []
    for i in range(8):
        a, b = rng.integers(-9, 10, size=3), rng.integers(-9, 10, size=3)
        if not a.any():
            a[i % 3] = 1
        if not b.any():
            b[(i + 1) % 3] = 1
        r.append(np.outer(a, b).astype(np.float64))
    for a, b in (([1, 0, 0], [1, 0, 0]), ([0, 0, 1], [0, 1, 0]), ([1, 1, 1], [1, -1, 1]), ([0, 3, 4], [2, 0, 0]), ([0, -1, 0], [0, 0, 7])):
        r.append(np.outer(a, b).astype(np.float64))
    fam["rank1"] = r
    # double and triple singular values: R is unique although U and V are not
    d = []
    for s in ((1.0, 1.0, 0.3), (1.0, 0.4, 0.4), (1.0, 1.0, 1.0), (1.0, 1.0, 1e-6)):
        for det in (1.0, -1.0):
            for rep in range(3):
                d.append(_usv(rng, s, det))
    for det in (1.0, -1.0):                         # exactly: a signed permutation, and 3 x the identity
        d.append(np.array([[0.0, 0.0, det], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]))
        d.append(3.0 * det * np.eye(3))
    fam["repeated"] = d
    # diagonal and permuted-diagonal: the Jacobi sweep meets zero off-diagonals (orthogonal columns) on entry
    g = []
    for trip in ((3.0, 2.0, 1.0), (3.0, -2.0, 1.0), (5.0, 5.0, -1.0), (1.0, 1e-4, 1e-8), (-1.0, 1e-9, 0.5)):
        for perm in itertools.permutations(range(3)):
            g.append(np.eye(3)[list(perm)] @ np.diag(trip))
    fam["diagonal"] = g
    return fam


def all_cases():
    """list of (family, label, M): every base matrix at SCALES; the zero matrix once"""
    out = []
    for name, mats in base_families().items():
        for i, M in enumerate(mats):
            for s in SCALES:
                out.append((name, "%s[%d]*%g" % (name, i, s), M * s))
    out.append(("zero", "zero", np.zeros((3, 3))))
    return out


def _mp(M):
    return mp.matrix([[mp.mpf(float(x)) for x in row] for row in np.asarray(M, dtype=np.float64)])


def _det3(A):
    """explicit: mpmath's det goes through an LU that does not survive a singular matrix"""
    return (A[0, 0] * (A[1, 1] * A[2, 2] - A[1, 2] * A[2, 1]) - A[0, 1] * (A[1, 0] * A[2, 2] - A[1, 2] * A[2, 0]) +
            A[0, 2] * (A[1, 0] * A[2, 1] - A[1, 1] * A[2, 0]))


def rule_rotation(U, Vt, proper):
    """the rotation of M = U diag(s) Vt (mp matrices) under either rule: U Vt times -1 where its determinant is negative (the
    reference), or U diag(1, 1, det U det Vt) Vt (`proper`)"""
    if proper:
        d = 1 if _det3(U) * _det3(Vt) > 0 else -1
        U = U.copy()
        for i in range(3):
            U[i, 2] = U[i, 2] * d
        return U * Vt
    R = U * Vt
    return R if _det3(R) > 0 else -R


def kind_of(s):
    """singular values (descending) -> "full" / "rank2" / "rank1" / "rank0", or "band" between determined and deficient"""
    if s[0] == 0:
        return "rank0"
    if s[2] >= FULL_MIN * s[0]:
        return "full"
    if s[2] <= DEFICIENT_MAX * s[0] and s[1] >= FULL_MIN * s[0]:
        return "rank2"
    if s[1] <= DEFICIENT_MAX * s[0]:
        return "rank1"
    return "band"


def reference(M):
    """60-digit SVD of the stored matrix: s (descending, mpf), kind ("full" / "rank2" / "rank1" / "rank0" / "band"), R (mp.matrix, or
    None for rank 1: no unique rotation)"""
    with mp.workdps(DPS):
        A = _mp(M)
        if not np.asarray(M).any():
            return dict(s=[mp.mpf(0)] * 3, kind="rank0", R=mp.eye(3))
        U, S, Vt = mp.svd_r(A)
        s = [S[i] for i in range(3)]
        assert s[0] >= s[1] >= s[2] >= 0
        kind = kind_of(s)
        R = None if kind in ("rank1", "band") else rule_rotation(U, Vt, proper=(kind == "rank2"))
    return dict(s=s, kind=kind, R=R)


EXPECTED_KIND = {"generic": "full", "mirrored": "full", "thin": "full", "repeated": "full", "diagonal": "full", "rank2": "rank2",
                 "rank1": "rank1", "zero": "rank0"}


def measure(M, R, ref):
    """dict of the normalised measures of the module's docstring (None where one does not apply) and `finite`"""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    res = dict(finite=bool(np.isfinite(R).all()), rot=None, orth=None, det=None, opt=None)
    if not res["finite"]:
        return res
    with mp.workdps(DPS):
        Rm = _mp(R)
        res["orth"] = float(max(abs(x) for x in (Rm.T * Rm - mp.eye(3))) / EPS)
        s = ref["s"]
        if ref["kind"] in ("full", "rank2"):
            res["rot"] = float(max(abs(x) for x in (Rm - ref["R"])) * (s[1] + s[2]) / (EPS * s[0]))
        if ref["kind"] == "rank1":
            res["det"] = float(abs(_det3(Rm) - 1) / EPS)
            tr = sum((Rm.T * _mp(M))[i, i] for i in range(3))
            res["opt"] = float(max(mp.mpf(0), s[0] - tr) / (EPS * s[0]))
    return res


def lapack(M, kind):
    """NumPy's float64 SVD on the same matrix with the rule of the case's kind"""
    U, _, Vt = np.linalg.svd(np.asarray(M, dtype=np.float64))
    if kind == "full":
        R = U @ Vt
        return -R if np.linalg.det(R) < 0 else R
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        U[:, 2] *= -1.0
    return U @ Vt


def check_case(family, label, M, R, ref, who, b=None):
    """every demand on a solver's result; returns the measures"""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    assert ref["kind"] == EXPECTED_KIND[family], "%s: the reference puts it at %s" % (label, ref["kind"])
    m = measure(M, R, ref)
    assert m["finite"], "%s %s: %r" % (who, label, R)
    if ref["kind"] == "rank0":
        assert (R == np.eye(3)).all(), "%s %s: %r" % (who, label, R)
        return m
    b = b or bounds(family)
    for key in MEASURES:
        if m[key] is not None:
            assert m[key] <= b[key], "%s %s: %s = %.4g (bound %.4g)" % (who, label, key, m[key], b[key])
    return m
