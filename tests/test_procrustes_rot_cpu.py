"""CPU: the 3 x 3 rotation solve of snapshot ingest (procrustes_rot, csrc/asb_kernels.h) through its host probe
asb_test_procrustes_rot, against a 60-digit SVD (mpmath) of the stored matrix.

Families (tests/procrustes_cases.py), each at scales 1e-150, 1e-8, 1, 1e8, 1e150: generic (s3 / s1 in [0.1, 1], det > 0), mirrored
(det < 0: the reference's -U V^T), thin (s3 / s1 = 1e-2 .. 1e-10, both signs), rank 2 (exact integer products: only the proper
rotation is accepted), rank 1 (finite, orthogonal, proper, optimal), double and triple singular values, diagonal and
permuted-diagonal matrices; the zero matrix gives the identity exactly.

Tolerances: procrustes_cases.LAPACK_WORST (the error of numpy.linalg.svd's U @ Vt on the same matrices, as literals) x 8, floored
at 16, in units of eps s1 / (s2 + s3) for R and of eps for R^T R - I, det R and the optimality gap; provenance in tests/README.md.
"""
import numpy as np
import pytest

import procrustes_cases as pc
from animsnapbases_amd import _lib

from procrustes_cases import LAPACK_WORST, MEASURES, check_case


@pytest.fixture(scope="module")
def cases():
    return [(fam, label, M, pc.reference(M)) for fam, label, M in pc.all_cases()]


def _host(M):
    M = np.ascontiguousarray(M, dtype=np.float64)
    out = np.full(11, -7.25)                      # two sentinels behind the nine results
    _lib.load().asb_test_procrustes_rot(M.ctypes.data, out.ctypes.data)
    assert (out[9:] == -7.25).all()
    return out[:9].reshape(3, 3).copy()


def test_every_case_is_on_its_side_of_the_rank_band(cases):
    """from the reference alone: full-rank families have s3 / s1 >= 1e-10, deficient ones <= 1e-15 for the first negligible singular
    value, nothing in between; both signs of det M and every scale occur among the thin cases"""
    count = {}
    for fam, label, M, ref in cases:
        assert ref["kind"] == pc.EXPECTED_KIND[fam], (label, ref["kind"], [float(x) for x in ref["s"]])
        s = ref["s"]
        if ref["kind"] == "full":
            assert s[2] >= pc.FULL_MIN * s[0], label
        elif ref["kind"] == "rank2":
            assert s[2] <= pc.DEFICIENT_MAX * s[0] and s[1] >= pc.FULL_MIN * s[0], label
        elif ref["kind"] == "rank1":
            assert s[1] <= pc.DEFICIENT_MAX * s[0] and s[0] > 0, label
        count[fam] = count.get(fam, 0) + 1
    assert set(count) == set(LAPACK_WORST) | {"zero"}
    thin = [(float(ref["s"][2] / ref["s"][0]), np.linalg.det(M / np.abs(M).max()) > 0) for fam, _, M, ref in cases if fam == "thin"]
    for r3 in pc.THIN:
        for positive in (True, False):
            assert sum(1 for r, p in thin if p == positive and r3 <= r <= 1.001 * r3) >= len(pc.SCALES), (r3, positive)
    # rank 2 comes both with s3 = 0 exactly and with s3 at rounding level
    s3 = [float(ref["s"][2] / ref["s"][0]) for fam, _, M, ref in cases if fam == "rank2"]
    assert min(s3) == 0.0 and max(s3) > 1e-18


def test_rotation_solve_against_60_digit_reference(cases):
    worst, checked, total = {}, {}, {}
    for fam, label, M, ref in cases:
        total[fam] = total.get(fam, 0) + 1
        m = check_case(fam, label, M, _host(M), ref, "procrustes_rot")
        checked[fam] = checked.get(fam, 0) + 1
        w = worst.setdefault(fam, dict.fromkeys(MEASURES, 0.0))
        for key in MEASURES:
            if m[key] is not None:
                w[key] = max(w[key], m[key])
    assert checked == total                       # no case skipped
    for fam in sorted(worst):
        print("procrustes_rot %-9s (%3d cases)" % (fam, total[fam]), " ".join("%s=%.3g" % (k, worst[fam][k]) for k in MEASURES))


def test_rank2_takes_the_proper_rotation_where_the_reference_rule_flips(cases):
    """the in-plane half-turn the reference's `R *= -1` produces when LAPACK's sign makes det(U V^T) negative is NOT what the solve
    returns: on every rank-2 case R maps the plane of the from-side onto the plane of the to-side with det R = +1 and
    tr(R^T M) = s1 + s2 (the half-turn would give s1 - s2 or less)"""
    n = 0
    for fam, label, M, ref in cases:
        if fam != "rank2":
            continue
        R = _host(M)
        sc = np.abs(M).max()
        s1, s2 = float(ref["s"][0] / sc), float(ref["s"][1] / sc)
        assert abs(np.linalg.det(R) - 1.0) <= 64 * pc.EPS, label
        assert abs(np.trace(R.T @ (M / sc)) - (s1 + s2)) <= 64 * pc.EPS * s1, label
        n += 1
    assert n == 16 * len(pc.SCALES)


def test_lapack_error_is_what_the_bars_were_derived_from(cases):
    """numpy.linalg.svd on the committed families against the same reference: its worst normalised errors are at or below the
    literals of procrustes_cases.LAPACK_WORST (a LAPACK that got worse would call for new bars, not silently looser ones) and not
    below half of them (the literals are LAPACK's, not padded)."""
    worst = {fam: [0.0] * 4 for fam in LAPACK_WORST}
    for fam, label, M, ref in cases:
        if fam == "zero":
            continue
        m = pc.measure(M, pc.lapack(M, ref["kind"]), ref)
        assert m["finite"], label
        for i, key in enumerate(MEASURES):
            if m[key] is not None:
                worst[fam][i] = max(worst[fam][i], m[key])
    for fam, lit in LAPACK_WORST.items():
        print("LAPACK %-9s" % fam, " ".join("%.4g" % x for x in worst[fam]))
        for got, want in zip(worst[fam], lit):
            assert 0.5 * want <= got <= want, (fam, worst[fam], lit)
