"""CPU: the host-callable pieces of the greedy step (csrc/asb_kernels.h) against exact references.

pick_cfg        every padded row length 16 .. 32768: the configuration covers the row, its block shape is consistent, and only
                the seven (T, E2) pairs that launch_stream instantiates ever come back.
eig3_top,       both symmetric 3 x 3 solvers against a 60-digit reference (mpmath) on families built to hit every branch
eig3_top_fast   (tests/eig3_cases.py): generic Gram matrices, exact rank 1 / 2, double and nearly double top eigenvalues, all three
                equal, diagonal matrices in every order, all of it at five scales and just under the solvers' 1e300 switch.

Tolerances: eig3_cases.LAPACK_WORST (LAPACK's measured error on the same matrices, as literals) x 8, floored at 16, in units of
eps max|a_ij| for lambda and the residual and of eps max|a_ij| / gap for the direction; provenance in tests/README.md.
"""
import numpy as np
import pytest

import eig3_cases as ec
from animsnapbases_amd import _lib

from eig3_cases import LAPACK_WORST, bounds, check_case

# Share of a family's cases that may go without a check, counted from the reference alone.
# Sign: skipped where the two largest magnitudes of u_ref are within 1e-8 of each other.
MAX_SIGN_SKIP = 0.10
# Direction: every case gets the angle (gap >= 1e-3 lambda_1) or the distance from the top cluster's eigen-space (below), except
# where all three eigenvalues are in the cluster and every unit vector is a top eigenvector to within 1e-3.  That is what the
# family `near_identity` is made of (lambda I and lambda (I + t E), t <= 1e-3: 174 of its 210 cases), so it has a limit of its
# own; there the residual bound is the direction check (|A u - lambda u| <= b eps max|a| puts u within b eps max|a| / gap of the
# eigenvector for any gap).  Everywhere else the limit is the 10 % of the sign rule (met by 4 of the 300 `double` cases only:
# third eigenvalue 0.999 lambda_1, at the edge of the cluster).
MAX_NO_DIRECTION = {"near_identity": 0.85}
MAX_NO_DIRECTION_DEFAULT = 0.10


@pytest.fixture(scope="module")
def cases():
    cs = ec.all_cases()
    return [(fam, label, a6, ec.reference(a6)) for fam, label, a6 in cs]


def _host(fn, a6):
    a6 = np.ascontiguousarray(a6, dtype=np.float64)
    out = np.full(6, -7.25)                       # two sentinels behind the four results
    getattr(_lib.load(), fn)(a6.ctypes.data, out.ctypes.data)
    assert (out[4:] == -7.25).all()
    return out[:4].copy()


def test_pick_cfg_covers_every_row_length_with_seven_configurations():
    lib = _lib.load()
    out = np.zeros(5, dtype=np.int32)
    seen = set()
    for Fp in range(16, 32768 + 1, 16):
        lib.asb_test_pick_cfg(Fp, out.ctypes.data)
        ok, T, E2, block, vpb = (int(x) for x in out)
        assert ok == 1, Fp
        assert 2 * T * E2 >= Fp, (Fp, T, E2)
        assert block == max(T, 256) and vpb * T == block, (Fp, T, E2, block, vpb)
        seen.add((T, E2))
    assert seen == {(64, 4), (128, 4), (256, 4), (512, 4), (1024, 4), (1024, 8), (1024, 16)}
    # each switch sits where the narrower configuration stops covering the row
    for Fp, want in ((512, (64, 4)), (528, (128, 4)), (1024, (128, 4)), (1040, (256, 4)), (2048, (256, 4)), (2064, (512, 4)),
                     (4096, (512, 4)), (4112, (1024, 4)), (8192, (1024, 4)), (8208, (1024, 8)), (16384, (1024, 8)),
                     (16400, (1024, 16)), (32768, (1024, 16))):
        lib.asb_test_pick_cfg(Fp, out.ctypes.data)
        assert (int(out[1]), int(out[2])) == want, Fp
    lib.asb_test_pick_cfg(32784, out.ctypes.data)
    assert out[0] == 0


def test_case_families_skip_little(cases):
    """counted from the reference alone: per family, the share of cases whose sign check is skipped and the share without a
    direction measure"""
    tot, skip, nodir = {}, {}, {}
    for fam, label, a6, ref in cases:
        tot[fam] = tot.get(fam, 0) + 1
        skip[fam] = skip.get(fam, 0) + int(ec.sign_skipped(ref))
        nodir[fam] = nodir.get(fam, 0) + int(fam != "zero" and len(ec.cluster_of(ref)) == 3)
    assert set(tot) == set(LAPACK_WORST) | {"zero"}
    for fam in tot:
        assert skip[fam] <= MAX_SIGN_SKIP * tot[fam], (fam, skip[fam], tot[fam])
        assert nodir[fam] <= MAX_NO_DIRECTION.get(fam, MAX_NO_DIRECTION_DEFAULT) * tot[fam], (fam, nodir[fam], tot[fam])
    # every branch of the direction check is populated: simple top eigenvalue, double, triple
    kinds = {len(ec.cluster_of(ref)) for fam, label, a6, ref in cases if fam != "zero"}
    assert kinds == {1, 2, 3}


@pytest.mark.parametrize("solver", ["asb_test_eig3", "asb_test_eig3_fast"])
def test_eig3_solvers_against_60_digit_reference(solver, cases):
    worst = {}
    for fam, label, a6, ref in cases:
        m = check_case(fam, label, a6, _host(solver, a6), ref, solver)
        w = worst.setdefault(fam, dict(lam=0.0, res=0.0, ang=0.0, sub=0.0))
        for key in w:
            if m[key] is not None:
                w[key] = max(w[key], m[key])
    for fam in sorted(worst):
        print("%s %-14s" % (solver, fam), " ".join("%s=%.3g" % kv for kv in sorted(worst[fam].items())))


def test_eig3_fast_agrees_with_jacobi_on_separated_spectra(cases):
    """where the top eigenvalue is simple both solvers return the same pair, sign included"""
    for fam, label, a6, ref in cases:
        if fam == "zero" or len(ec.cluster_of(ref)) != 1 or ec.sign_skipped(ref):
            continue
        a, b = _host("asb_test_eig3", a6), _host("asb_test_eig3_fast", a6)
        bd = bounds(fam)
        gap = float(ref["lam"][0] - ref["lam"][1])
        assert abs(a[0] - b[0]) <= 2 * bd["lam"] * ec.EPS * ref["sc"], label
        assert np.abs(a[1:] - b[1:]).max() <= 2 * bd["ang"] * ec.EPS * ref["sc"] / gap + 4 * ec.EPS, label


def test_lapack_error_is_what_the_bars_were_derived_from(cases):
    """numpy.linalg.eigh on the committed families against the same reference: its worst normalised errors are at or below the
    literals of eig3_cases.LAPACK_WORST (a LAPACK that got worse would call for new bars, not silently looser ones) and not
    below half of them (the literals are LAPACK's, not padded)."""
    worst = {fam: [0.0] * 4 for fam in LAPACK_WORST}
    for fam, label, a6, ref in cases:
        if fam == "zero":
            continue
        m = ec.measure(a6, ec.lapack(a6), ref)
        assert m["finite"], label
        for i, key in enumerate(("lam", "res", "ang", "sub")):
            if m[key] is not None:
                worst[fam][i] = max(worst[fam][i], m[key])
    for fam, lit in LAPACK_WORST.items():
        print("LAPACK %-14s" % fam, " ".join("%.4g" % x for x in worst[fam]))
        for got, want in zip(worst[fam], lit):
            assert 0.5 * want <= got <= want, (fam, worst[fam], lit)
