"""60-digit model (mpmath) of "project F" -- the second half of the strain and deformation-gradient projections of
csrc/asb_cproj.hip (cp_project_tri / cp_project_tet, csrc/asb_cproj_elem.h) -- and the error measures shared by
tests/test_cproj_model_cpu.py (host probe, LAPACK) and tests/test_gpu_cproj_edges.py (device probe, k_cproj, k_cproj_em).
Not a test module.

The expected result is computed from the STORED float64 matrix F = U diag(s) W^T (mpmath SVD, s descending), by the rank the
reference alone decides (`rank_of`: s_k / s_1 >= 1e-10 counts, <= 1e-50 is zero, anything between is an error of the inputs),
with c = clip(s, sigma_min, sigma_max) and c_n = clip(0, sigma_min, sigma_max):

  full rank   tets_strain                U diag(c) W^T, c_3 negated where det F < 0 (Constraint_projections.py:547-553)
              tets_deformation_gradient  R = U W^T, its third column negated where det R < 0; the kernel stores R^T (:682-687)
              tris_strain                Fhat = U diag(c) W^T (2 x 2); the kernel stores (P Fhat)^T (:411-425)
  one zero    det F = 0: not inverted.  The null pair (u_n, w_n) is fixed up to a common sign by det U det W = +1, so
              strain: sum_(i < n) c_i u_i w_i^T + c_n u_n w_n^T;  deformation gradient: U diag(1, 1, det U det W) W^T
  3 x 3, two zeros   no unique result: properties only (`measure`)
  F = 0       c_n I, and I for the deformation gradient

Conditioning of the strain kinds.  Fhat = U g(S) W^T is a function of F alone; with E = U^T dF W, to first order (the
Daleckii-Krein formula for the singular value decomposition)
    (U^T dFhat W)_ii = g'(s_i) E_ii
    (U^T dFhat W)_ij = (g_i - g_j) / (s_i - s_j) * (E_ij + E_ji) / 2  +  (g_i + g_j) / (s_i + s_j) * (E_ij - E_ji) / 2      (i != j)
g = clip is monotone and 1-Lipschitz, so g' and every (g_i - g_j) / (s_i - s_j) lie in [0, 1]; only the skew coefficients can
exceed 1.  An error of e |F| in F therefore moves Fhat by at most e s_1 kappa,
    kappa = max(1, max_(i < j) (c_i + c_j) / (s_i + s_j))                                                    not inverted.
On an inverted element write F = U' diag(s_1, s_2, -s_3) W^T with det U' det W = +1: the reference's result is
U' diag(c_1, c_2, c_3) W^T, the same formula with the SIGNED third value -s_3 mapped to +c_3.  The pairs (i, 3) then have the
coefficients (c_i - c_3) / (s_i + s_3), at most 1 in size, and (c_i + c_3) / (s_i - s_3):
    kappa = max(1, (c_1 + c_2) / (s_1 + s_2), (c_1 + c_3) / (s_1 - s_3), (c_2 + c_3) / (s_2 - s_3))           inverted
-- the pair (1, 3) enters as well as (2, 3).  The rule is discontinuous where an inverted element has s_2 = s_3; the families
keep s_2 - s_3 >= 0.1 s_1 there.  The rotation U W^T has the polar factor's conditioning 2 / (s_2 + s_3) per unit of |dF|
(R.-C. Li, SIAM J. Matrix Anal. Appl. 16 (1995)), whatever the sign of det F.

Measures, in units of eps = 2^-52 (None where one does not apply):
    err   strain kinds, unique result:  max|Fhat - ref| / (kappa max(c_1, s_1))
    rot   deformation gradient, unique: max|R - ref| (s_2 + s_3) / (2 s_1)
    orth  deformation gradient:         max|R^T R - I|
    det   deformation gradient:         |det R - 1|     (proper in every rank: the reference's column flip on a full-rank F,
                                        det U det W = +1 on a deficient one)
  3 x 3 with two zero singular values, m = max(c_1, s_1):
    sv    strain: max|singular values of Fhat - sort(c_1, c_n, c_n)| / m
    map   strain: max|Fhat w_1 - c_1 u_1| / m;   deformation gradient: max|R w_1 - u_1|
    neg   strain: max(0, -det Fhat) / m^3
    dist  strain: | |Fhat - F|_F - sqrt((c_1 - s_1)^2 + 2 c_n^2) | / m
"""
import mpmath as mp
import numpy as np

EPS = 2.0 ** -52
DPS = 60
FULL_MIN = 1e-10            # a singular value of at least this x s_1 counts
DEFICIENT_MAX = 1e-50       # one of at most this x s_1 is zero; nothing may lie between
KINDS = {"tris_strain": 1, "tets_strain": 2, "tets_deformation_gradient": 3}          # the codes of the C ABI
MEASURES = ("err", "rot", "orth", "det", "sv", "map", "neg", "dist")


def _mp(M):
    return mp.matrix([[mp.mpf(float(x)) for x in row] for row in np.asarray(M, dtype=np.float64)])


def _det(A):
    """explicit: mpmath's det goes through an LU that does not survive a singular matrix"""
    if A.rows == 2:
        return A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
    return (A[0, 0] * (A[1, 1] * A[2, 2] - A[1, 2] * A[2, 1]) - A[0, 1] * (A[1, 0] * A[2, 2] - A[1, 2] * A[2, 0]) +
            A[0, 2] * (A[1, 0] * A[2, 1] - A[1, 1] * A[2, 0]))


def rank_of(s):
    """singular values (descending) -> the number that count, or None for one in the band between full and deficient"""
    if s[0] == 0:
        return 0
    r = 0
    for x in s:
        if x >= FULL_MIN * s[0]:
            r += 1
        elif x > DEFICIENT_MAX * s[0]:
            return None
    return r


def decompose(M):
    """the clamp-independent part, once per stored matrix: dict(n, A, U, Wt, s (mpf, descending), rank, inverted, dUW)"""
    M = np.asarray(M, dtype=np.float64)
    n = M.shape[0]
    with mp.workdps(DPS):
        A = _mp(M)
        if not M.any():
            return dict(n=n, A=A, U=mp.eye(n), Wt=mp.eye(n), s=[mp.mpf(0)] * n, rank=0, inverted=False, dUW=1)
        U, S, Wt = mp.svd_r(A)
        s = [S[i] for i in range(n)]
        assert all(s[i] >= s[i + 1] >= 0 for i in range(n - 1))
        rank = rank_of(s)
        dUW = 1 if _det(U) * _det(Wt) > 0 else -1
        return dict(n=n, A=A, U=U, Wt=Wt, s=s, rank=rank, inverted=(rank == n and dUW < 0), dUW=dUW)


def _clip(x, lo, hi):
    return min(max(x, mp.mpf(lo)), mp.mpf(hi))


def _usw(U, d, Wt):
    n = U.rows
    D = mp.zeros(n)
    for i in range(n):
        D[i, i] = d[i]
    return U * D * Wt


def expected(dec, kind, smin, smax):
    """dict(ref (mp.matrix in the orientation of `oriented`, or None where the result is not unique), c, cn, kappa)"""
    n, s, rank = dec["n"], dec["s"], dec["rank"]
    assert rank is not None, "a singular value between full rank and deficient"
    assert n == (2 if kind == "tris_strain" else 3)
    with mp.workdps(DPS):
        cn = _clip(mp.mpf(0), smin, smax)
        c = [_clip(x, smin, smax) if i < rank else cn for i, x in enumerate(s)]
        unique = rank >= n - 1 or rank == 0
        if kind == "tets_deformation_gradient":
            ref = None
            if rank == n:
                ref = dec["U"] * dec["Wt"]
                if _det(ref) < 0:
                    for i in range(3):
                        ref[i, 2] = -ref[i, 2]
            elif unique:
                ref = _usw(dec["U"], [1, 1, dec["dUW"]] if rank else [1, 1, 1], dec["Wt"])
            return dict(ref=ref, c=c, cn=cn, kappa=None)
        sg = list(s)
        d = list(c)
        if dec["inverted"] and n == 3:                   # (the 2 x 2 clamp has no inversion rule)
            d[2], sg[2] = -d[2], -sg[2]
        elif 0 < rank < n:
            d[n - 1] = d[n - 1] * dec["dUW"]
        ref = _usw(dec["U"], d, dec["Wt"]) if unique else None
        kappa = mp.mpf(1)
        if rank:
            for i in range(n):
                for j in range(i + 1, n):
                    if sg[i] + sg[j] > 0:
                        kappa = max(kappa, (c[i] + c[j]) / (sg[i] + sg[j]))
        return dict(ref=ref, c=c, cn=cn, kappa=kappa)


def oriented(kind, out):
    """the kernels' / probes' output of one element as the matrix the measures speak of: R for the deformation gradient (stored
    as R^T), Fhat otherwise"""
    out = np.asarray(out, dtype=np.float64)
    return out.T if kind == "tets_deformation_gradient" else out


def _amax(A):
    return max(abs(x) for x in A)


def measure(dec, exp, kind, out):
    """dict over MEASURES (None where one does not apply) and `finite`; `out` as the probes return it"""
    X = oriented(kind, out)
    res = dict.fromkeys(MEASURES)
    res["finite"] = bool(np.isfinite(X).all())
    if not res["finite"]:
        return res
    n, s, rank = dec["n"], dec["s"], dec["rank"]
    with mp.workdps(DPS):
        Xm = _mp(X)
        e = mp.mpf(EPS)
        if kind == "tets_deformation_gradient":
            res["orth"] = float(_amax(Xm.T * Xm - mp.eye(3)) / e)
            res["det"] = float(abs(_det(Xm) - 1) / e)
            if exp["ref"] is not None and rank:
                res["rot"] = float(_amax(Xm - exp["ref"]) * (s[1] + s[2]) / (2 * s[0]) / e)
            elif rank == 1:
                u1 = dec["U"][:, 0]
                w1 = dec["Wt"][0, :].T
                res["map"] = float(_amax(Xm * w1 - u1) / e)
            return res
        m = max(exp["c"][0], s[0])
        if exp["ref"] is not None:
            res["err"] = float(_amax(Xm - exp["ref"]) / (exp["kappa"] * m) / e) if m > 0 else float(_amax(Xm - exp["ref"]))
            return res
        c1, cn = exp["c"][0], exp["cn"]
        sv = mp.svd_r(Xm, compute_uv=False)
        want = sorted([c1, cn, cn], reverse=True)
        res["sv"] = float(max(abs(sv[i] - want[i]) for i in range(3)) / m / e)
        u1 = dec["U"][:, 0]
        w1 = dec["Wt"][0, :].T
        res["map"] = float(_amax(Xm * w1 - c1 * u1) / m / e)
        res["neg"] = float(max(mp.mpf(0), -_det(Xm)) / m ** 3 / e)
        D = Xm - dec["A"]
        res["dist"] = float(abs(mp.sqrt(sum(x * x for x in D)) - mp.sqrt((c1 - s[0]) ** 2 + 2 * cn ** 2)) / m / e)
    return res


def lapack(kind, M, smin, smax, rank):
    """`projections.project_host`'s formula on one matrix in float64 -- numpy.linalg.svd, the clip, the reference's two sign rules --
    with the deficient-rank rule applied to its U: the last column changes sign where det U det Vt < 0, and a deficient F is not
    inverted.  The sign of det F comes from slogdet, which neither overflows nor flushes to zero at the extreme scales.  Returned
    in the probes' orientation."""
    M = np.asarray(M, dtype=np.float64)
    n = M.shape[0]
    U, s, Vt = np.linalg.svd(M)
    if rank < n and np.linalg.det(U) * np.linalg.det(Vt) < 0:
        U[:, n - 1] *= -1.0
    if kind == "tets_deformation_gradient":
        R = U @ Vt
        if np.linalg.det(R) < 0:
            R[:, 2] *= -1.0
        return R.T
    c = np.clip(s, smin, smax)
    if kind == "tets_strain" and rank == 3 and np.linalg.slogdet(M)[0] < 0:
        c[2] = -c[2]
    return (U * c) @ Vt
