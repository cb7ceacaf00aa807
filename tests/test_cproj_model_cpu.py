"""CPU: "project F" of the constraint projections (cp_project_tri / cp_project_tet, csrc/asb_cproj_elem.h -- the routines the
kernels k_cproj and k_cproj_em call) through the host probe asb_test_cproj_project, against the 60-digit model of
tests/cproj_model.py on the families of tests/cproj_cases.py: flat (rank 2), collapsed (rank 1, F = 0), inverted, thin, graded
and repeated singular values, every position of the clamp, each at the scales 2^-400 .. 2^400.

Tolerances: cproj_cases.LAPACK_WORST (the error of numpy.linalg.svd in the reference's formula on the same matrices, as
literals) x 8, floored at 16, in the units of cproj_model's measures; provenance in tests/README.md.

On the routines as they stood before this file (absolute `sig > 0` test, u_j = v_j, `al * be` unscaled) the host probe failed
tets_strain / tets_deformation_gradient on rank2, rank1, and every family at 2^266 and 2^400, and tris_strain on rank1 and
the same scales; the counts are in tests/README.md."""
import numpy as np
import pytest

import cproj_cases as cc
import cproj_model as cm
from conftest import load_golden

KINDS = ("tets_strain", "tets_deformation_gradient", "tris_strain")


@pytest.fixture(scope="module")
def cases():
    """n -> list of (family, label, F, lo, hi, decomposition)"""
    return {n: [(fam, label, F, lo, hi, cm.decompose(F)) for fam, label, F, lo, hi in cc.all_cases(n)] for n in (2, 3)}


host = cc.host_probe


def test_every_case_is_on_its_side_of_the_rank_band(cases):
    """from the model alone: full-rank families have s_n / s_1 >= 1e-10, deficient ones <= 1e-50 for every vanished singular
    value, nothing in between; inverted 3 x 3 cases have s_2 - s_3 >= 0.1 s_1; both signs of det and every scale occur in thin"""
    for n in (2, 3):
        count, inverted = {}, 0
        for fam, label, F, lo, hi, dec in cases[n]:
            s, rank = dec["s"], dec["rank"]
            assert rank == cc.expected_rank(n, fam), (label, rank, [float(x) for x in s])
            for i in range(n):
                if i < rank:
                    assert s[i] >= cm.FULL_MIN * s[0], label
                else:
                    assert s[i] <= cm.DEFICIENT_MAX * s[0], label
            if n == 3 and dec["inverted"]:
                inverted += 1
                assert s[1] - s[2] >= 0.1 * s[0], label
            assert lo <= hi
            count[fam] = count.get(fam, 0) + 1
        assert set(count) == set(cc.LAPACK_WORST["tets_strain" if n == 3 else "tris_strain"]) | {"zero"}
        assert n == 2 or inverted >= 6 * len(cc.SCALES)
        thin = [(float(dec["s"][n - 1] / dec["s"][0]), dec["dUW"] > 0) for fam, _, _, _, _, dec in cases[n] if fam == "thin"]
        for r in (cc.THIN3 if n == 3 else cc.THIN2):
            for positive in (True, False):
                assert sum(1 for x, p in thin if p == positive and r <= x <= 1.001 * r) >= len(cc.SCALES), (n, r, positive)
    assert sum(len(v) for v in cases.values()) <= 706                  # no more than the Procrustes table


@pytest.mark.parametrize("kind", KINDS)
def test_host_probe_against_60_digit_model(cases, kind):
    worst, checked, total = {}, {}, {}
    for fam, label, F, lo, hi, dec in cases[cc.DIM[kind]]:
        total[fam] = total.get(fam, 0) + 1
        m = cc.check_case(kind, fam, label, F, lo, hi, host(kind, F, lo, hi), dec, cm.expected(dec, kind, lo, hi), "host probe")
        checked[fam] = checked.get(fam, 0) + 1
        w = worst.setdefault(fam, {})
        for key in cm.MEASURES:
            if m[key] is not None:
                w[key] = max(w.get(key, 0.0), m[key])
    assert checked == total                         # no case skipped
    for fam in sorted(worst):
        print("host %s %-9s (%3d cases)" % (kind, fam, total[fam]), " ".join("%s=%.3g" % kv for kv in sorted(worst[fam].items())))


@pytest.mark.parametrize("kind", KINDS)
def test_lapack_error_is_what_the_bars_were_derived_from(cases, kind):
    """numpy.linalg.svd in the reference's formula on the committed families against the same model: its worst normalised errors
    are at or below the literals of cproj_cases.LAPACK_WORST (a LAPACK that got worse would call for new bars, not silently
    looser ones) and above half of them (the literals are LAPACK's, not padded)."""
    worst = {}
    for fam, label, F, lo, hi, dec in cases[cc.DIM[kind]]:
        if fam == "zero":
            continue
        m = cm.measure(dec, cm.expected(dec, kind, lo, hi), kind, cm.lapack(kind, F, lo, hi, dec["rank"]))
        assert m["finite"], label
        w = worst.setdefault(fam, {})
        for key in cm.MEASURES:
            if m[key] is not None:
                w[key] = max(w.get(key, 0.0), m[key])
    for fam in sorted(worst):
        print("LAPACK %s %r: {%s}," % (kind, fam, ", ".join('"%s": %.3g' % kv for kv in sorted(worst[fam].items()))))
    assert set(worst) == set(cc.LAPACK_WORST[kind])
    for fam, lit in cc.LAPACK_WORST[kind].items():
        assert set(lit) == set(worst[fam]), (fam, sorted(worst[fam]))
        for key, want in lit.items():
            got = worst[fam][key]               # (a literal 0: exact to the model's own 60 digits)
            assert 0.5 * want < got <= want or (want == 0.0 and got < 1e-30), (kind, fam, key, got, want)


# ---------------------------------------------------------------- the model is the reference's operation
def _fixture_F(name):
    """the float64 deformation gradients of a well-conditioned fixture of the unmodified reference, (F, e, n, n), and its
    expected projections as (F, e, n, n) in the probes' orientation"""
    g = load_golden("cproj_" + name)
    rest, el, fr = g["rest"], g["elements"], g["frames"]
    if name == "tris_strain":
        P, DmInv = g["P"], g["DmInv"]
        Ds = np.stack([fr[:, el[:, 1]] - fr[:, el[:, 0]], fr[:, el[:, 2]] - fr[:, el[:, 0]]], axis=3)
        Fm = np.einsum("tij,ftik->ftjk", P, Ds) @ DmInv[None]
        pi = g["expected"].reshape(fr.shape[0], el.shape[0], 2, 3)                 # (P Fhat)^T
        return g, Fm, np.einsum("ftac,tcb->ftba", pi, P), P                        # Fhat = P^T pi^T
    p4 = rest[el[:, 3]]
    Dm = np.stack([rest[el[:, 0]] - p4, rest[el[:, 1]] - p4, rest[el[:, 2]] - p4], axis=2)
    x4 = fr[:, el[:, 3]]
    Ds = np.stack([fr[:, el[:, 0]] - x4, fr[:, el[:, 1]] - x4, fr[:, el[:, 2]] - x4], axis=3)
    return g, Ds @ np.linalg.inv(Dm)[None], g["expected"].reshape(fr.shape[0], el.shape[0], 3, 3), None


@pytest.mark.parametrize("kind", KINDS)
def test_model_reproduces_the_fixtures_of_the_unmodified_reference(kind):
    """tests/golden/cproj_<kind>.npz holds what the reference's classes returned.  On a sample of its (frame, element) pairs --
    every inverted one of the first frames among them -- the model, fed the float64 F formed from the fixture's positions, gives
    the fixture's projection to 1e-12, the tolerance test_gpu_cproj.py holds the kernel to (kappa <= 1e3 there): the model is
    the reference's operation, not a restatement of the kernel."""
    g, Fm, want, P = _fixture_F(kind)
    lo, hi = float(g["sigma"][0]), float(g["sigma"][1])
    nF, ne = Fm.shape[:2]
    pairs = [(f, e) for f in range(0, nF, 13) for e in range(0, ne, 7)]
    if kind != "tris_strain":
        inv = np.argwhere(np.linalg.det(Fm) < 0)
        assert len(inv) >= 10
        pairs += [tuple(x) for x in inv[:12]]
    worst = 0.0
    for f, e in pairs:
        dec = cm.decompose(Fm[f, e])
        assert dec["rank"] == cc.DIM[kind]
        ref = np.array(cm.expected(dec, kind, lo, hi)["ref"].tolist(), dtype=np.float64)
        worst = max(worst, np.abs(cm.oriented(kind, want[f, e]) - ref).max())
        # and the host probe on the same F
        assert np.abs(host(kind, Fm[f, e], lo, hi) - want[f, e]).max() <= 1e-12
    print("%s: %d pairs, model against fixture %.3g" % (kind, len(pairs), worst))
    assert worst <= 1e-12
