"""Deformation gradients for "project F" of the constraint projections (csrc/asb_cproj_elem.h): the families, the bars and the
check shared by tests/test_cproj_model_cpu.py and tests/test_gpu_cproj_edges.py.  The expected values and the measures are
tests/cproj_model.py's.  Not a test module.

A case is (family, label, F, sigma_min, sigma_max).  F is built from chosen factors U diag(s) V^T with s_1 = 1, rounded once,
or -- the deficient families -- as an exact product of small integers over 128; the expected result is computed from what was
stored.  Every base case is then multiplied by each of SCALES, F and its clamp alike (powers of two: the scaled case is an exact
image of the base case, and the integer families stay exactly deficient), so that the same singular values are inside, below
and above the clamp at every scale.  Families other than `clamp` use CLAMP = [0.25, 0.75] x scale: with s_1 = 1 .. 3 the largest
singular value is clipped from above, small ones from below, and the rest pass.

  3 x 3 (tets_strain and tets_deformation_gradient)
    generic    s_3 / s_1 in [0.1, 1], det > 0
    mirrored   det < 0 with s_2 - s_3 >= 0.1 s_1 (the reference's rule is discontinuous at s_2 = s_3 there)
    thin       s_3 / s_1 = 1e-2 .. 1e-10, both signs of det
    graded     s = (1, 1e-5, 1e-10)
    repeated   s_1 = s_2 (both signs), s_2 = s_3 and all equal (det > 0), signed permutations
    clamp      s = (1, 0.6, 0.3), both signs: every sigma inside, below, above; both bounds active; sigma_min = sigma_max = 1;
               sigma_min = 0; a bound one ulp above and one ulp below an exact sigma, and on the rounded sigma_3 of a generic F
    rank2      exact integer products; a zero row (all four corners in a coordinate plane), a zero column (a corner on the
               fourth); two equal / opposite rows of generic doubles
    rank1      exact integer outer products, zero rows and columns among them
    diagonal   diagonal and permuted-diagonal: orthogonal columns on entry
    zero       F = 0
  2 x 2 (tris_strain): generic, mirrored, thin (1e-2, 1e-6, 1e-10), repeated, clamp, rank1, diagonal, zero
"""
import numpy as np

import cproj_model as cm

EPS = cm.EPS
SCALES = (2.0 ** -400, 2.0 ** -27, 1.0, 2.0 ** 27, 2.0 ** 266, 2.0 ** 400)
KERNEL_SCALES = (2.0 ** -27, 1.0, 2.0 ** 27)        # the real kernels: world positions of an animation
CLAMP = (0.25, 0.75)
THIN3 = (1e-2, 1e-4, 1e-6, 1e-8, 1e-10)
THIN2 = (1e-2, 1e-6, 1e-10)
DIM = {"tris_strain": 2, "tets_strain": 3, "tets_deformation_gradient": 3}
DEFICIENT = {(3, "rank2"): 2, (3, "rank1"): 1, (2, "rank1"): 1, (3, "zero"): 0, (2, "zero"): 0}      # expected rank; others full

# Tolerances.  The reference's solver for this step is LAPACK (numpy.linalg.svd in `get_pi`), so the bar is LAPACK's own error
# on the same matrices against the same 60-digit model: cproj_model.lapack, measured once (figures in tests/README.md).  Per kind,
# family and measure 8 x LAPACK's worst, never below 16.  LAPACK's worst, rounded up to three digits;
# test_cproj_model_cpu.py::test_lapack_error_is_what_the_bars_were_derived_from measures them again:
LAPACK_WORST = {
    "tets_strain": {
        "generic": {"err": 2.5},
        "mirrored": {"err": 1.08},
        "thin": {"err": 8.69},
        "graded": {"err": 0.128},
        "repeated": {"err": 9.93},
        "clamp": {"err": 2.5},
        "rank2": {"err": 1.56},
        "rank1": {"sv": 3.24, "map": 2.45, "neg": 0.0, "dist": 3.4},
        "diagonal": {"err": 0.334},
    },
    "tets_deformation_gradient": {
        "generic": {"rot": 2.12, "orth": 6.48, "det": 7.18},
        "mirrored": {"rot": 2.42, "orth": 8.17, "det": 8.13},
        "thin": {"rot": 6.23, "orth": 4.55, "det": 3.58},
        "graded": {"rot": 0.128, "orth": 2.85, "det": 3.01},
        "repeated": {"rot": 7.12, "orth": 4.09, "det": 3.89},
        "clamp": {"rot": 1.1, "orth": 4.04, "det": 3.91},
        "rank2": {"rot": 1.24, "orth": 4.05, "det": 2.55},
        "rank1": {"orth": 5.0, "det": 6.0, "map": 3.2},
        "diagonal": {"rot": 0.251, "orth": 1.0, "det": 1.0},
    },
    "tris_strain": {
        "generic": {"err": 1.01},
        "mirrored": {"err": 1.22},
        "thin": {"err": 1.38},
        "repeated": {"err": 0.888},
        "clamp": {"err": 0.5},
        "rank1": {"err": 1.1},
        "diagonal": {"err": 0.0},
    },
}
MARGIN, FLOOR = 8.0, 16.0


def bounds(kind, family):
    return {k: max(MARGIN * w, FLOOR) for k, w in LAPACK_WORST[kind][family].items()}


def _rand_orth(rng, n, det):
    Q, R = np.linalg.qr(rng.normal(size=(n, n)))
    Q = Q * np.sign(np.diag(R))
    if np.linalg.det(Q) * det < 0:
        Q[:, n - 1] *= -1
    return Q


def _usv(rng, s, det):
    """U diag(s) V^T with det U det V = det, rounded once"""
    n = len(s)
    du = 1.0 if rng.random() < 0.5 else -1.0
    return (_rand_orth(rng, n, du) * np.asarray(s, dtype=np.float64)) @ _rand_orth(rng, n, du * det).T


def _perm(n, p, signs):
    return np.eye(n)[list(p)] * np.asarray(signs, dtype=np.float64)


def _base3():
    rng = np.random.default_rng(20241020)
    fam = {}
    fam["generic"] = []
    for i in range(6):
        r3 = rng.uniform(0.1, 1.0)
        fam["generic"].append((_usv(rng, (1.0, rng.uniform(r3, 1.0), r3), 1.0),) + CLAMP)
    fam["mirrored"] = []
    for i in range(6):
        r3 = rng.uniform(0.1, 0.8)
        fam["mirrored"].append((_usv(rng, (1.0, rng.uniform(r3 + 0.1, 1.0), r3), -1.0),) + CLAMP)
    # a hair above r3, so that rounding F (which moves s_3 by up to eps s_1) keeps 1e-10 on the full-rank side
    fam["thin"] = [(_usv(rng, (1.0, rng.uniform(0.2, 1.0), r3 * (1.0 + 1e-4)), det),) + CLAMP for r3 in THIN3 for det in (1.0, -1.0)]
    fam["graded"] = [(_usv(rng, (1.0, 1e-5, 1e-10 * (1.0 + 1e-4)), 1.0),) + CLAMP for i in range(3)]
    rep = [(_usv(rng, s, det),) + CLAMP for s, dets in (((1.0, 1.0, 0.3), (1.0, -1.0)), ((1.0, 0.4, 0.4), (1.0, 1.0)),
                                                          ((1.0, 1.0, 1.0), (1.0, 1.0)), ((0.5, 0.5, 1e-6), (1.0, -1.0)))
           for det in dets]
    rep.append((_perm(3, (2, 0, 1), (1, 1, 1)),) + CLAMP)                       # det +1
    rep.append((_perm(3, (1, 0, 2), (1, -1, 1)),) + CLAMP)                      # det +1
    rep.append((0.5 * np.eye(3),) + CLAMP)                                      # inside the clamp: Fhat = F
    rep.append((_perm(3, (0, 2, 1), (-1, 1, 1)) * 3.0,) + CLAMP)                # det +1
    fam["repeated"] = rep
    cl = []
    for det in (1.0, -1.0):
        M = _usv(rng, (1.0, 0.6, 0.3), det)
        for lo, hi in ((0.1, 2.0), (1.5, 2.0), (0.05, 0.2), (0.5, 0.8), (1.0, 1.0), (0.0, 0.8)):
            cl.append((M, lo, hi))
    D = _perm(3, (1, 2, 0), (1, -1, 1)) @ np.diag([1.0, 0.6, 0.3])             # singular values exactly 1, 0.6, 0.3
    cl.append((D, np.nextafter(0.3, 1.0), np.nextafter(0.6, 0.0)))              # each bound one ulp inside an exact sigma
    cl.append((D, np.nextafter(0.3, 0.0), np.nextafter(0.6, 1.0)))              # ... and one ulp outside
    G = fam["generic"][0][0]
    s3 = float(cm.decompose(G)["s"][2])
    cl.append((G, s3, 5.0))                                                     # sigma_min = the rounded sigma_3
    fam["clamp"] = cl
    # rank 2 exactly: (3 x 2 integers) (2 x 3 integers) / 128
    r = []
    while len(r) < 4:
        A, B = rng.integers(-9, 10, size=(3, 2)), rng.integers(-9, 10, size=(2, 3))
        if np.linalg.matrix_rank(A) == 2 and np.linalg.matrix_rank(B) == 2:
            r.append(A @ B)
    r.append(np.array([[3, 1, -2], [-1, 2, 5], [0, 0, 0]]))                     # all four corners in the plane z = 0
    r.append(np.array([[1, 0, 4], [2, 0, -3], [-5, 0, 1]]))                     # corner 2 on corner 4
    r.append(np.array([[0, 0, 0], [0, 7, 0], [0, 0, 2]]))                       # a zero row and a zero column
    r.append(np.array([[1, 2], [2, 1], [3, 3]]) @ np.array([[1, 0, 0], [0, 1, 0]]))
    fam["rank2"] = [(M.astype(np.float64) / 128.0,) + CLAMP for M in r]
    # two rows equal or opposite, of generic doubles (a tet pressed onto the plane x = y or x = -y): exactly rank 2, but the
    # float64 determinant is a rounding residue of either sign
    rr = np.random.default_rng(5)
    for t in range(6):
        r0, r2 = rr.uniform(-1, 1, 3), rr.uniform(-1, 1, 3)
        if t >= 3:                                  # (of the first three draws the residue is zero or positive)
            fam["rank2"].append((np.array([r0, r0 if t % 2 == 0 else -r0, r2]),) + CLAMP)
    # rank 1 exactly: outer products of small integer vectors / 64
    r = []
    for i in range(4):
        a, b = rng.integers(-9, 10, size=3), rng.integers(-9, 10, size=3)
        a[i % 3] = a[i % 3] or 1
        b[(i + 1) % 3] = b[(i + 1) % 3] or 1
        r.append(np.outer(a, b))
    for a, b in (([1, 0, 0], [1, 0, 0]), ([0, 0, 1], [0, 1, 0]), ([1, 1, 1], [1, -1, 1]), ([0, 3, 4], [2, 0, 5])):
        r.append(np.outer(a, b))
    fam["rank1"] = [(M.astype(np.float64) / 64.0,) + CLAMP for M in r]
    g = []
    for trip, perm in (((1.0, 0.5, 0.125), (0, 1, 2)), ((1.0, -0.5, 0.125), (1, 2, 0)), ((1.25, 1.25, -0.25), (2, 1, 0)),
                       ((1.0, 1e-4, 1e-8), (1, 2, 0)), ((-1.0, 1e-9, 0.5), (2, 0, 1)), ((0.5, 0.625, -0.375), (1, 0, 2))):
        g.append((np.eye(3)[list(perm)] @ np.diag(trip),) + CLAMP)
    fam["diagonal"] = g
    return fam


def _base2():
    rng = np.random.default_rng(20241021)
    fam = {}
    fam["generic"] = [(_usv(rng, (1.0, rng.uniform(0.1, 1.0)), 1.0),) + CLAMP for i in range(4)]
    fam["mirrored"] = [(_usv(rng, (1.0, rng.uniform(0.1, 1.0)), -1.0),) + CLAMP for i in range(4)]
    fam["thin"] = [(_usv(rng, (1.0, r2 * (1.0 + 1e-4)), det),) + CLAMP for r2 in THIN2 for det in (1.0, -1.0)]
    fam["repeated"] = [(_usv(rng, (1.0, 1.0), 1.0),) + CLAMP, (_usv(rng, (1.0, 1.0), -1.0),) + CLAMP,
                       (np.array([[0.0, -1.0], [1.0, 0.0]]),) + CLAMP, (np.array([[0.0, 1.0], [1.0, 0.0]]),) + CLAMP,
                       (0.5 * np.eye(2),) + CLAMP]
    M = _usv(rng, (1.0, 0.4), 1.0)
    cl = [(M, lo, hi) for lo, hi in ((0.1, 2.0), (1.5, 2.0), (0.05, 0.2), (0.5, 0.8), (1.0, 1.0), (0.0, 0.8))]
    D = np.array([[0.0, -0.4], [1.0, 0.0]])
    cl.append((D, np.nextafter(0.4, 1.0), np.nextafter(1.0, 0.0)))
    cl.append((D, np.nextafter(0.4, 0.0), np.nextafter(1.0, 2.0)))
    fam["clamp"] = cl
    r = []
    for i in range(3):
        a, b = rng.integers(-9, 10, size=2), rng.integers(-9, 10, size=2)
        a[i % 2] = a[i % 2] or 1
        b[(i + 1) % 2] = b[(i + 1) % 2] or 1
        r.append(np.outer(a, b))
    # (the last two: the sweep leaves a residue in the vanished column, where the others leave an exact zero)
    for a, b in (([1, 0], [1, 0]), ([0, 1], [1, 0]), ([1, 1], [1, -1]), ([3, 4], [0, 2]), ([-9, 4], [2, 7]), ([-9, 5], [-4, 9])):
        r.append(np.outer(a, b))
    fam["rank1"] = [(M.astype(np.float64) / 64.0,) + CLAMP for M in r]
    fam["diagonal"] = [(np.eye(2)[list(p)] @ np.diag(d),) + CLAMP
                       for d, p in (((1.0, -0.5), (1, 0)), ((-1.0, 1e-9), (0, 1)), ((1e-4, 1.0), (1, 0)), ((-0.375, 0.625), (0, 1)))]
    return fam


def base_families(n):
    """family -> list of (F, sigma_min, sigma_max) at scale 1, n = 2 or 3"""
    return _base3() if n == 3 else _base2()


def all_cases(n, scales=SCALES):
    """list of (family, label, F, sigma_min, sigma_max): every base case at every scale; the zero matrix with the clamp at scale 1"""
    out = []
    for name, cases in base_families(n).items():
        for i, (M, lo, hi) in enumerate(cases):
            for k in scales:
                out.append((name, "%s[%d]*2^%d" % (name, i, int(np.log2(k))), M * k, lo * k, hi * k))
    out.append(("zero", "zero", np.zeros((n, n))) + CLAMP)
    out.append(("zero", "zero, sigma_min = 0", np.zeros((n, n)), 0.0, 1.0))
    return out


def host_probe(kind, F, lo, hi):
    """asb_test_cproj_project on one matrix"""
    from animsnapbases_amd import _lib
    F = np.ascontiguousarray(F, dtype=np.float64)
    out = np.full(F.size + 2, -7.25)                # two sentinels behind the result
    rc = _lib.load().asb_test_cproj_project(cm.KINDS[kind], F.ctypes.data, 1, float(lo), float(hi), out.ctypes.data)
    assert rc == 0 and (out[F.size:] == -7.25).all()
    return out[:F.size].reshape(F.shape).copy()


def expected_rank(n, family):
    return DEFICIENT.get((n, family), n)


def check_case(kind, family, label, F, lo, hi, out, dec, exp, who, b=None):
    """every demand on one result (as the probes return it); returns the measures"""
    n = DIM[kind]
    assert dec["rank"] == expected_rank(n, family), "%s: the model puts it at rank %r" % (label, dec["rank"])
    m = cm.measure(dec, exp, kind, out)
    assert m["finite"], "%s %s %s: %r" % (who, kind, label, out)
    if dec["rank"] == 0:
        want = np.eye(n) * (1.0 if kind == "tets_deformation_gradient" else float(exp["cn"]))
        assert np.array_equal(np.asarray(out), want), "%s %s %s: %r" % (who, kind, label, out)
        return m
    b = b or bounds(kind, family)
    for key in cm.MEASURES:
        if m[key] is not None:
            assert m[key] <= b[key], "%s %s %s: %s = %.4g (bar %.4g)" % (who, kind, label, key, m[key], b[key])
    return m
