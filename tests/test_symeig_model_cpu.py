"""CPU: the model, the cases and the bars of the symmetric eigen-solver's tests (symeig_model.py, symeig_cases.py), and
the defect that the split-matrix repair of k_tri_shifts / k_tri_invit removed, shown on float64 transcriptions of the two
routines: the span measures fail on the old one (OLD_FAILURES: family -> count) and pass on the repaired one."""
import collections

import numpy as np
import pytest

import symeig_cases as C
import symeig_model as M

LD = M.LD
MEASURES = ("lam", "res", "unit", "sub", "ritz")


@pytest.fixture(scope="module")
def tri():
    """every tridiagonal case with its reference and LAPACK's pairs, computed once"""
    out = []
    for c in C.tri_cases():
        A = M.dense_of(c["d"], c["e"])
        lam, U = M.reference(A)
        ll, lv = M.lapack_tri(c["d"], c["e"])
        out.append((c, A, lam, U, ll, lv))
    return out


@pytest.fixture(scope="module")
def dense():
    out = []
    for c in C.dense_cases():
        lam, U = M.reference(c["A"])
        out.append((c, lam, U) + M.lapack_dense(c["A"]))
    return out


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("n", [1, 2, 3, 64, 130])
def test_bisection_meets_the_closed_form(n):
    d, e = C.toeplitz121(n)
    lam, _ = C.toeplitz121_pairs(n, np.arange(n))
    assert np.abs(M.sturm_eigs(d, e)[::-1] - lam).max() <= 16 * np.finfo(LD).eps * 4


def test_householder_is_a_similarity_and_reads_back_from_storage():
    rng = np.random.default_rng(1)
    A = rng.normal(size=(40, 40))
    A = 0.5 * (A + A.T)
    A[:, 7] = A[7, :] = 0.0
    A[7, 7] = 1.0
    A[20:, :20] = A[:20, 20:] = 0.0                          # two blocks: reflectors with tau == 0 at the boundary
    d, e, V, tau = M.householder(A)
    assert np.sum(tau == 0) >= 2 and e[19] == 0
    Q = M.backtransform(V, tau, np.eye(40))
    T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
    assert np.abs(Q @ T @ Q.T - A).max() <= 1e-17 * np.abs(A).max() * 40
    assert np.abs(Q.T @ Q - np.eye(40)).max() <= 1e-17 * 40
    stored = np.zeros((40, 40))
    for j in range(38):
        stored[j, j + 1:] = V[j, j + 1:].astype(np.float64)     # what asb_sym_tridiag leaves in row j
    V2, tau2 = M.reflectors_of(stored)
    assert np.array_equal(tau2 == 0, tau == 0) and np.abs(tau2 - tau).max() <= 8 * M.EPS


def test_reference_vectors_are_accurate_beyond_float64(dense):
    for c, lam, U, *_ in dense:
        if c["label"] in ("random-65", "arrowhead-130", "tridiagonal-64"):
            A = c["A"].astype(LD)
            assert np.abs(A @ U - U * lam[None]).max() <= 1e-17 * float(np.abs(lam).max()), c["label"]
            assert np.abs(U.T @ U - np.eye(len(lam))).max() <= 1e-17


# ---------------------------------------------------------------------------------------------------------------- the cases
def test_every_case_is_what_its_family_says(tri, dense):
    for c, A, lam, U, ll, lv in tri:
        assert C.tri_predicate(c, lam), c["label"]
    for c, lam, U, *_ in dense:
        assert C.dense_predicate(c, lam), c["label"]
    labels = [t[0]["label"] for t in tri] + ["dense " + t[0]["label"] for t in dense]
    assert len(labels) == len(set(labels))


def test_cases_cover_the_edges(tri, dense):
    fams = {t[0]["family"] for t in tri}
    assert fams == {"toeplitz", "wilkinson", "glued", "multiple", "zero", "split", "tiny_e", "graded", "gram"}
    for fam in fams - {"wilkinson", "glued", "split"}:
        assert {len(t[0]["d"]) for t in tri if t[0]["family"] == fam} >= set(C.TRI_SIZES) - ({1, 2} if fam == "gram" else set())
    assert {k for t in tri for k in t[0]["ks"]} >= {1, 63, 64, 65, 130}
    glued = {t[0]["label"] for t in tri if t[0]["family"] == "glued" and "x2^" not in t[0]["label"]}
    assert glued == {"W%d+x%d-glue%g" % (w, c, g) for w, c in ((21, 5), (21, 12), (61, 4)) for g in C.GLUES}
    assert {t[0]["label"] for t in tri if t[0]["family"] == "wilkinson"} >= {"W21+", "W61+", "W101+"}
    split = {t[0]["label"] for t in tri if t[0]["family"] == "split"}
    assert split >= {"period3-30", "blocks-32x2", "blocks-21x3", "six", "order1-between"}
    for fam in fams - {"zero"}:                                                       # both ends of the exponent range
        assert any(t[0]["label"].endswith("x2^-400") for t in tri if t[0]["family"] == fam), fam
        assert any(t[0]["label"].endswith("x2^400") for t in tri if t[0]["family"] == fam), fam
    dfams = {t[0]["family"] for t in dense}
    assert dfams == {"random", "lowrank", "plateau", "circulant", "kron", "kron_perm", "diagonal", "tridiagonal", "arrowhead", "rank1",
                     "isolated", "zero"}
    for fam in dfams - {"kron", "kron_perm"}:
        assert {t[0]["A"].shape[0] for t in dense if t[0]["family"] == fam} >= set(C.DENSE_SIZES), fam
    assert any(t[0].get("zero_e") for t in dense) and any(t[0].get("t_is_a") for t in dense)
    assert any(t[0]["label"].startswith("kron3") for t in dense)
    # at size: every route of csrc/asb_eig.hip that the rest of the suite does not reach
    R = {(n, k): C.routes(n, k) for n in C.AT_SIZE for k in C.AT_SIZE_KS[n]}
    assert set(C.AT_SIZE) == {256, 258, 322, 1537, 4200, 5089, 6785, 10177}
    assert {r["wpb"] for r in R.values() if r["back"] == "wave"} == {1, 2, 3, 4}
    assert R[(5089, 3)]["wpb"] == 3 and C.routes(5088, 3)["wpb"] == 4 and R[(6785, 3)]["wpb"] == 2 and C.routes(6784, 3)["wpb"] == 3
    assert R[(10177, 1)]["wpb"] == 1 and C.routes(10176, 1)["wpb"] == 2
    blocked = {n: r for (n, k), r in R.items() if r["back"] == "blocked"}
    assert blocked[256]["groups"] == 4 and blocked[256]["last_group"] == 62            # the smallest blocked shape, k = 2
    assert blocked[258]["last_group"] == 64 and blocked[322]["last_group"] == 64       # nrefl a whole multiple of 64
    assert R[(10177, 2)]["back"] == "wave"                                             # odd n: never blocked
    assert R[(1537, 2)]["panels"] >= 1 and R[(256, 2)]["panels"] == 0
    assert max(r["panels"] for r in R.values()) > C.routes(2601, 2)["panels"]          # k_td_panel above the suite's largest n
    assert R[(10177, 1)]["panel_chunks"] == 10 and R[(4200, 2)]["panel_chunks"] > 3
    # behind the panels the two-launch loop only ever sees the last 544 columns: k_td_small_reg<4>, one chunk.  The large-block
    # forms run when the panels are off (ASB_TD_PANEL_MIN=0) or have fallen back:
    assert all(r["small"] == {"reg4"} and r["update_chunks"] == 1 for (n, k), r in R.items() if n >= C.PANEL_MIN)
    loop = C.routes(C.NO_PANEL, 1, panels=False)
    assert loop["small"] == {"small", "reg8", "reg4"} and loop["update_chunks"] == 10 and loop["panels"] == 0


# ---------------------------------------------------------------------------------------------------------------- the bars
def _round_up3(x):
    if x == 0:
        return 0.0
    p = 10.0 ** (np.floor(np.log10(x)) - 2)
    return float(np.ceil(x / p) * p)


def tri_figures(tri):
    """LAPACK's worst figure per family and measure, and the share of the vectors that sit in a cluster cut by k"""
    worst = collections.defaultdict(lambda: dict.fromkeys(MEASURES + ("rank",), 0.0))
    cut, tot = collections.Counter(), collections.Counter()
    for c, A, lam, U, ll, lv in tri:
        for k in c["ks"]:
            m = M.measure(A, ll, lv[:, :k], lam, U, k)
            for q in worst[c["family"]]:
                worst[c["family"]][q] = max(worst[c["family"]][q], m[q])
            cut[c["family"]] += m["cut"]
            tot[c["family"]] += k
    return worst, {f: cut[f] / tot[f] for f in tot}


def dense_figures(dense):
    worst = collections.defaultdict(lambda: dict.fromkeys(MEASURES + ("rank", "tri"), 0.0))
    cut, tot = collections.Counter(), collections.Counter()
    for c, lam, U, ll, lv, d, e in dense:
        f = c["family"]
        worst[f]["tri"] = max(worst[f]["tri"], M.tri_error(d, e, lam))
        for k in c["ks"]:
            m = M.measure(c["A"], ll, lv[:, :k], lam, U, k)
            for q in MEASURES + ("rank",):
                worst[f][q] = max(worst[f][q], m[q])
            cut[f] += m["cut"]
            tot[f] += k
    return worst, {f: cut[f] / tot[f] for f in tot}


def at_size_figures(n):
    """LAPACK on the permuted 1-2-1 matrix of order n (numpy.linalg.eigh, scipy.linalg.hessenberg) against the closed form"""
    from scipy.linalg import hessenberg
    A, p = C.perm121(n)
    ll, lv = np.linalg.eigh(A)
    ll, lv = ll[::-1].copy(), lv[:, ::-1]
    out = dict.fromkeys(MEASURES + ("tri",), 0.0)
    for k in C.AT_SIZE_KS[n]:
        lam, U = C.perm121_reference(n, p, k)
        m = M.measure(lambda X: C.perm121_matvec(p, X), ll, lv[:, :k], lam, U, k)
        for q in MEASURES:
            out[q] = max(out[q], m[q])
    H = hessenberg(A)
    out["tri"] = M.tri_error(np.diag(H), np.diag(H, 1), lam)
    return out


def _check_literals(worst, literals):
    for fam, fig in worst.items():
        for q, x in fig.items():
            if q == "rank":
                assert x <= 1 + 1e-12                                   # LAPACK's vectors have condition 1
                continue
            lit = literals[fam][q]
            assert x <= lit and (x > 0.5 * lit or lit == 0.0), (fam, q, x, lit)


def test_lapack_error_is_what_the_bars_were_derived_from(tri, dense):
    """Bar = max(8 x LAPACK's worst, 16) per family and measure.  LAPACK's worst figures are literals (C.LAPACK_TRI,
    C.LAPACK_DENSE, C.LAPACK_AT_SIZE, rounded up to three digits); here they are measured again: at or below the literal, above
    half of it.  At size LAPACK was run once per n up to 4200; this test repeats it up to 1537.  For 5089 .. 10177 the figure of
    4200 is scaled by sqrt(n / 4200): the rounding errors of independent reflectors add like a random walk."""
    worst, share = tri_figures(tri)
    _check_literals(worst, C.LAPACK_TRI)
    dworst, dshare = dense_figures(dense)
    _check_literals(dworst, C.LAPACK_DENSE)
    # clusters cut by k are not compared vector by vector; outside the families that ARE one repeated value they stay under 10 %
    for f, s in list(share.items()) + list(dshare.items()):
        assert s <= 0.10 or f in ("multiple", "zero", "diagonal"), (f, s)
    for n in C.AT_SIZE:
        if n <= 1537:
            _check_literals({n: at_size_figures(n)}, C.LAPACK_AT_SIZE)
    for n in (5089, 6785, 10177):
        for q in MEASURES + ("tri",):
            assert C.at_size_bar(n, q) == max(16.0, 8 * C.LAPACK_AT_SIZE[4200][q] * np.sqrt(n / 4200.0))


# ---------------------------------------------------------------------------------------------------------------- old and new
OLD_FAILURES = {"multiple": 33, "zero": 12, "split": 42}            # (family: number of (case, k) that miss a span bar)


def _span_failures(tri, blocks):
    fails, flagged = collections.Counter(), 0
    for c, A, lam, U, ll, lv in tri:
        if c["family"] == "glued":
            continue                                                # unreduced deep clusters: a documented limit (tests/README.md)
        for k in c["ks"]:
            lam_got, Z, bad = M.invit_f64(c["d"], c["e"], ll, k, blocks)
            m = M.measure(A, lam_got, Z, lam, U, k)
            lit = C.LAPACK_TRI[c["family"]]
            ok = np.isfinite(Z).all() and m["rank"] <= M.RANK_BAR and all(m[q] <= C.bar(lit[q]) for q in MEASURES)
            fails[c["family"]] += not ok
            flagged += bad
    return {f: x for f, x in fails.items() if x}, flagged


def test_the_old_routine_fails_the_span_measures_and_the_repaired_one_passes(tri):
    """k_tri_shifts + k_tri_invit transcribed to float64 (eigenvalues from LAPACK): before the repair every family with exact
    zeros in e loses the span -- identical vectors from one start vector -- while every residual stays below eps |T|."""
    old, _ = _span_failures(tri, blocks=False)
    assert old == OLD_FAILURES
    new, flagged = _span_failures(tri, blocks=True)
    assert new == {} and flagged == 0


def test_the_glued_family_is_a_documented_limit(tri):
    """Unreduced clusters deeper than inverse iteration separates without re-orthogonalisation: the repaired routine still loses
    rank on glued Wilkinson matrices (not asked of it); lam, res, unit hold."""
    worst = 0.0
    for c, A, lam, U, ll, lv in tri:
        if c["family"] != "glued":
            continue
        k = c["ks"][-1]
        lam_got, Z, bad = M.invit_f64(c["d"], c["e"], ll, k, True)
        m = M.measure(A, lam_got, Z, lam, U, k)
        lit = C.LAPACK_TRI["glued"]
        assert bad == 0 and all(m[q] <= C.bar(lit[q]) for q in ("lam", "res", "unit")), (c["label"], m)
        worst = max(worst, m["rank"])
    assert worst > M.RANK_BAR


if __name__ == "__main__":                                           # prints the literals of symeig_cases.py
    import sys
    if sys.argv[1:] == ["at-size"]:
        print("LAPACK_AT_SIZE = {")
        for n in C.AT_SIZE:
            if n <= 4200:
                print("    %d: %r," % (n, {q: _round_up3(x) for q, x in at_size_figures(n).items()}), flush=True)
        print("}")
    else:
        t = [(c, M.dense_of(c["d"], c["e"])) + M.reference(M.dense_of(c["d"], c["e"])) + M.lapack_tri(c["d"], c["e"]) for c in C.tri_cases()]
        w, s = tri_figures(t)
        print("LAPACK_TRI = {")
        for f in w:
            print("    %r: %r," % (f, {q: _round_up3(x) for q, x in w[f].items() if q != "rank"}))
        print("}", s)
        dn = [(c,) + M.reference(c["A"]) + M.lapack_dense(c["A"]) for c in C.dense_cases()]
        w, s = dense_figures(dn)
        print("LAPACK_DENSE = {")
        for f in w:
            print("    %r: %r," % (f, {q: _round_up3(x) for q, x in w[f].items() if q != "rank"}))
        print("}", s)
        if C.LAPACK_TRI:
            print(_span_failures(t, False), _span_failures(t, True))
