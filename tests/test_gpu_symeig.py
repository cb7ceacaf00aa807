"""GPU (-m gpu): the symmetric eigen-solver behind the constraint POD, phase by phase against the longdouble model of
symeig_model.py on the cases of symeig_cases.py:

1. bisection + inverse iteration (asb_test_tridiag_eig) on every tridiagonal family -- split matrices, multiple and
   clustered eigenvalues, graded and scaled ones;
2. the Householder tridiagonalisation alone (asb_sym_tridiag);
3. the back-transformation alone on a prescribed Z (asb_sym_backtransform), blocked and one wave per column;
4. the whole chain (asb_sym_eig_topk) on every dense family;
5. the permuted 1-2-1 matrix at the sizes where asb_eig.hip changes kernels;
6. the constraint POD end to end on frames whose Gram matrix splits, is a multiple of the identity, or is circulant.

Measures and bars: symeig_model.measure, symeig_cases.bar -- max(8 x LAPACK's worst, 16) in units of eps max|lambda| per
family and measure, cond(V) <= 2^20.  Every check prints its figures before it asserts (pytest -s)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import symeig_cases as C
import symeig_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MEASURES = ("lam", "res", "unit", "sub", "ritz")
GLUED_ASSERTED = ("lam", "res", "unit")          # the rest of `glued` is a documented limit (tests/README.md): printed only

TRI_CASES = C.tri_cases()
DENSE_CASES = C.dense_cases()
TRI_FAMILIES = sorted({c["family"] for c in TRI_CASES})
DENSE_FAMILIES = sorted({c["family"] for c in DENSE_CASES})
_REF = {}


def ref_of(label, A):
    """the longdouble reference of a case: computed once, shared, never modified"""
    if label not in _REF:
        lam, U = M.reference(A)
        lam.setflags(write=False)
        U.setflags(write=False)
        _REF[label] = (lam, U)
    return _REF[label]


@pytest.fixture(scope="module")
def eng():
    from animsnapbases_amd import HipEngine
    e = HipEngine(0, stream=0)
    yield e
    e.close()


def _show(label, k, m, bad=0):
    print("%-30s k=%3d bad=%d %s" % (label, k, bad, " ".join("%s=%.3g" % (q, m[q]) for q in m if q != "descending")))


def _misses(label, k, m, literals, which=MEASURES, rank=True):
    """the measures of one (case, k) that miss their bar: every case of a family is measured and printed before the test asserts"""
    out = [(label, k, q, round(m[q], 3), C.bar(literals[q])) for q in which if not m[q] <= C.bar(literals[q])]
    if rank and not m["rank"] <= M.RANK_BAR:
        out.append((label, k, "rank", m["rank"], M.RANK_BAR))
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. tridiagonal
def check_tri_family(eng, family):
    """also run by test_gpu_dense_blocks._child_tridiag under ASB_TRI_MULTISECT=0"""
    misses = []
    for c in [c for c in TRI_CASES if c["family"] == family]:
        A = M.dense_of(c["d"], c["e"])
        ref_lam, ref_U = ref_of("tri " + c["label"], A)
        for k in c["ks"]:
            lam, Z, bad = eng.test_tridiag_eig(c["d"], c["e"], k)
            assert np.isfinite(lam).all() and np.isfinite(Z).all(), (c["label"], k)
            m = M.measure(A, lam, Z, ref_lam, ref_U, k)
            _show(c["label"], k, m, bad)
            assert bad == 0 and m["descending"], (c["label"], k, bad)
            glued = family == "glued"
            misses += _misses(c["label"], k, m, C.LAPACK_TRI[family], GLUED_ASSERTED if glued else MEASURES, rank=not glued)
            if not np.any(c["d"]) and not np.any(c["e"]):
                assert not np.any(lam)                                       # the zero matrix: lam == 0 exactly
            if not np.any(c["e"]):
                assert np.array_equal(lam, np.sort(c["d"])[::-1])            # a diagonal matrix: its entries, exactly
                assert np.array_equal(np.sort(np.abs(Z).ravel())[-k:], np.ones(k)) and np.count_nonzero(Z) == k
            # a vector never leaves the block that owns its eigenvalue
            starts = M.split_starts(c["d"], c["e"])
            for v in range(k):
                nz = np.flatnonzero(Z[:, v])
                b = np.searchsorted(starts, nz[0], side="right") - 1
                assert starts[b] <= nz[0] and nz[-1] < starts[b + 1], (c["label"], k, v)
            if c["label"].startswith("blocks-") and k == len(c["d"]):
                assert identical_blocks_agree(Z, starts), c["label"]
    assert not misses, misses


def identical_blocks_agree(Z, starts):
    """Identical blocks take identical arithmetic -- shifts are pushed apart within a block only, so another block's equal
    eigenvalue changes nothing: the vectors of every copy are those of the first, bit for bit."""
    parts = []
    for s0, s1 in zip(starts[:-1], starts[1:]):
        cols = [v for v in range(Z.shape[1]) if np.any(Z[s0:s1, v])]
        parts.append(Z[s0:s1][:, cols])
    return all(p.shape == parts[0].shape and np.array_equal(p, parts[0]) for p in parts[1:])


@pytest.mark.parametrize("family", TRI_FAMILIES)
def test_tridiagonal_families(eng, family):
    check_tri_family(eng, family)


def test_unsplit_input_is_bit_identical_to_the_parent_commit(eng):
    """tests/golden/symeig_gram_like.npz: d, e of the gram-like family and what asb_test_tridiag_eig returned for them before
    the split-matrix repair (MI355X).  An unsplit T takes the same arithmetic, operation for operation."""
    g = np.load(os.path.join(HERE, "golden", "symeig_gram_like.npz"))
    for n, k in ((3, 3), (64, 20), (65, 65), (130, 64)):
        d, e = g["d%d" % n], g["e%d" % n]
        assert np.all(e != 0)
        lam, Z, bad = eng.test_tridiag_eig(d, e, k)
        assert bad == 0 and np.array_equal(lam, g["lam%d" % n]) and np.array_equal(Z, g["Z%d" % n]), n


# ---------------------------------------------------------------------------------------------------------------- 2. reduction
def _tridiag(eng, A):
    import torch
    Ad = torch.from_numpy(np.array(A, dtype=np.float64, order="C")).cuda()
    d, e = eng.sym_tridiag(A.shape[0], Ad.data_ptr())
    return Ad, d, e


@pytest.mark.parametrize("family", DENSE_FAMILIES)
def test_tridiagonalisation_alone(eng, family):
    for c in [c for c in DENSE_CASES if c["family"] == family]:
        A = c["A"]
        ref_lam, _ = ref_of("dense " + c["label"], A)
        _, d, e = _tridiag(eng, A)
        assert np.isfinite(d).all() and np.isfinite(e).all()
        tri = M.tri_error(d, e, ref_lam)
        print("%-30s tri=%.3g" % (c["label"], tri))
        assert tri <= C.bar(C.LAPACK_DENSE[family]["tri"]), (c["label"], tri)
        if c.get("t_is_a"):                                                   # every tau == 0: T == A bit for bit
            assert np.array_equal(d, np.diag(A)) and np.array_equal(e, np.diag(A, 1)), c["label"]
        for j in c.get("zero_e", []):                                          # a block boundary stays an exact zero
            assert e[j] == 0.0, (c["label"], j, e[j])


# ---------------------------------------------------------------------------------------------------------------- 3. Q Z
BACK_CASES = [("perm121", 256), ("perm121", 258), ("perm121", 322), ("kron2", 256), ("perm121", 130), ("kron2", 64), ("random", 65)]


def back_bar(n):
    """|Q Z - model|_2 per column in units of eps: a reflector applied to a unit column leaves a rounding error of about 4 eps
    (an ordered dot product and one update per entry); n - 2 independent ones add like a random walk, 4 sqrt(n); four times that."""
    return 16.0 * np.sqrt(n)


def _back_matrix(kind, n):
    if kind == "perm121":
        return C.perm121(n)[0]
    if kind == "kron2":
        return C.kron_gram(2, n // 2, 900 + n)                     # reflectors with tau == 0 inside a group of 64
    rng = np.random.default_rng(n)
    B = rng.normal(size=(n, n))
    return 0.5 * (B + B.T)


def check_backtransform(eng, kind, n):
    """also run by test_gpu_dense_blocks._child_eigensolver under ASB_BACKTRANSFORM_BLOCKED=0: the same (n, k), the other route"""
    Ad, d, e = _tridiag(eng, _back_matrix(kind, n))
    V, tau = M.reflectors_of(Ad.cpu().numpy())
    if kind == "kron2":
        assert np.sum(tau == 0) >= 2 and e[n // 2 - 1] == 0.0
    rng = np.random.default_rng(n + 1)
    for k in (2, 3, 64, 65):
        for name, Z in (("identity", np.eye(n)[:, :k]), ("random", np.linalg.qr(rng.normal(size=(n, k)))[0])):
            got = eng.sym_backtransform(n, Z, Ad.data_ptr())
            want = M.backtransform(V, tau, Z)
            D = got.astype(M.LD) - want
            err = float(np.sqrt((D * D).sum(axis=0)).max() / M.EPS)
            route = C.routes(n, k, blocked=os.environ.get("ASB_BACKTRANSFORM_BLOCKED", "1") != "0")["back"]
            print("%s-%d k=%d %s %s: %.3g eps (bar %.3g)" % (kind, n, k, name, route, err, back_bar(n)))
            assert np.isfinite(got).all() and err <= back_bar(n), (kind, n, k, name, err)


@pytest.mark.parametrize("kind,n", BACK_CASES)
def test_backtransformation_alone(eng, kind, n):
    check_backtransform(eng, kind, n)


def check_backtransform_all(eng=None):
    from animsnapbases_amd import HipEngine
    e = eng or HipEngine(0, stream=0)
    try:
        for kind, n in BACK_CASES:
            check_backtransform(e, kind, n)
    finally:
        if eng is None:
            e.close()


# ---------------------------------------------------------------------------------------------------------------- 4. the chain
@pytest.mark.parametrize("family", DENSE_FAMILIES)
def test_whole_chain(eng, family):
    """asb_sym_eig_topk on every dense case, all measures."""
    import torch
    misses = []
    for c in [c for c in DENSE_CASES if c["family"] == family]:
        A, n = c["A"], c["A"].shape[0]
        ref_lam, ref_U = ref_of("dense " + c["label"], A)
        for k in c["ks"]:
            Ad = torch.from_numpy(A.copy()).cuda()
            lam, V, bad = eng.sym_eig_topk(n, k, Ad.data_ptr(), want_vectors=True)
            assert np.isfinite(lam).all() and np.isfinite(V).all(), (c["label"], k)
            m = M.measure(A, lam, V, ref_lam, ref_U, k)
            _show(c["label"], k, m, bad)
            assert bad == 0 and m["descending"], (c["label"], k, bad)
            misses += _misses(c["label"], k, m, C.LAPACK_DENSE[family])
            if not np.any(A):
                assert not np.any(lam) and np.abs(V.T @ V - np.eye(k)).max() <= 16 * M.EPS
    assert not misses, misses


# ---------------------------------------------------------------------------------------------------------------- 5. at size
def check_at_size(eng, n, panels=True):
    import torch
    A, p = C.perm121(n)
    Ad = torch.from_numpy(A).cuda()
    d, e = eng.sym_tridiag(n, Ad.data_ptr())
    assert np.isfinite(d).all() and np.isfinite(e).all()
    lam_all = C.toeplitz121_lam(n)
    # tri, as two Sturm counts in longdouble: the i-th eigenvalue of the device's T lies within the bar of the i-th reference value
    w = C.at_size_bar(n, "tri") * M.EPS * 4
    asc = lam_all[::-1]
    assert np.all(M.sturm_count(d, e, asc - w) <= np.arange(n)) and np.all(M.sturm_count(d, e, asc + w) >= np.arange(n) + 1), n
    for k in C.AT_SIZE_KS[n]:
        lam, Z, bad = eng.test_tridiag_eig(d, e, k)
        V = eng.sym_backtransform(n, Z, Ad.data_ptr())
        ref_lam, ref_U = C.perm121_reference(n, p, k)
        m = M.measure(lambda X: C.perm121_matvec(p, X), lam, V, ref_lam, ref_U, k)
        _show("perm121-%d %s" % (n, C.routes(n, k, panels=panels)), k, m, bad)
        assert bad == 0 and m["descending"] and np.isfinite(V).all()
        miss = [(n, k, q, m[q], C.at_size_bar(n, q)) for q in MEASURES if not m[q] <= C.at_size_bar(n, q)]
        assert not miss and m["rank"] <= M.RANK_BAR, (miss, m["rank"])


@pytest.mark.parametrize("n", C.AT_SIZE)
def test_at_size(eng, n):
    """The 1-2-1 matrix under a fixed permutation (integer entries, closed-form pairs) where asb_eig.hip changes route:
    symeig_cases.routes names the kernels of each (n, k).  n = 10177 is reduced once, k = 1 and 2 on the same T."""
    check_at_size(eng, n)


def _child_no_panels():
    from animsnapbases_amd import HipEngine
    e = HipEngine(0, stream=0)
    try:
        check_at_size(e, C.NO_PANEL, panels=False)
    finally:
        e.close()
    print("no panels: n = %d OK" % C.NO_PANEL)


def test_at_size_two_launch_loop_from_the_first_column():
    """ASB_TD_PANEL_MIN=0 (read once per process): k_td_small above 8192 rows, k_td_small_reg<8>, <4> and k_td_update with ten
    column chunks -- behind the panel kernel the loop only ever sees the last 544 columns."""
    env = dict(os.environ, ASB_TD_PANEL_MIN="0")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_symeig as t; t._child_no_panels()" % (ROOT, HERE)
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    print(p.stdout.decode())
    assert p.returncode == 0 and "OK" in p.stdout.decode(), (p.returncode, p.stderr.decode(errors="replace")[-4000:])


# ---------------------------------------------------------------------------------------------------------------- 6. end to end
def _frames(kind):
    rng = np.random.default_rng(17)
    ep = 60
    if kind == "mirrored":                        # a motion on one vertex set, then the same on a disjoint one: G = kron(I_2, B)
        m = 60
        Mo = rng.normal(size=(m, ep // 2, 3)) * (0.9 ** np.arange(m))[:, None, None]
        fr = np.zeros((1 + 2 * m, ep, 3))
        fr[1:1 + m, :ep // 2] = Mo
        fr[1 + m:, ep // 2:] = Mo
        return fr, 40
    if kind == "orthogonal":                      # orthogonal frames of equal norm: G = c I
        F = 129
        Q, _ = np.linalg.qr(rng.normal(size=(3 * ep, F)))
        return np.concatenate([np.zeros((1, ep, 3)), Q.T.reshape(F, ep, 3)]), 32
    F = 128                                       # a looping animation: G circulant, every singular value twice
    t = 2 * np.pi * np.arange(F) / F
    fr = np.zeros((F, ep, 3))
    for h in range(1, 25):
        a, b = rng.normal(size=(2, ep, 3)) * 0.8 ** h
        fr += np.cos(h * t)[:, None, None] * a + np.sin(h * t)[:, None, None] * b
    return np.concatenate([np.zeros((1, ep, 3)), fr]), 30


@pytest.mark.parametrize("kind", ["mirrored", "orthogonal", "looping"])
def test_pod_end_to_end_on_split_equal_and_circulant_gram_matrices(kind, tmp_path):
    """constraintsComponents' POD against numpy.linalg.svd of X with the assertions of
    test_pod_clustered_spectrum_vs_lapack_on_A: singular values to 1e-10, an orthonormal basis, clusters as subspaces to 1e-5."""
    from conftest import relerr
    from test_gpu_smalldense import _pod
    frames, K = _frames(kind)
    ns, cc = _pod(frames, K, tmp_path)
    X = ((frames - frames[0:1]) * ns.pre_scale_factor).reshape(frames.shape[0], -1).T
    Ur, Sr, _ = np.linalg.svd(X, full_matrices=False)
    print(kind, "singular values", relerr(cc.singular_values[:K], Sr[:K]))
    assert relerr(cc.singular_values[:K], Sr[:K]) < 1e-10
    got = cc.comps.reshape(K, -1).T
    assert np.allclose(got.T @ got, np.eye(K), atol=1e-10)
    k = 0
    while k < K:
        j = k + 1
        while j < K and Sr[k] - Sr[j] < 1e-6 * Sr[k]:
            j += 1
        if j >= K and j < len(Sr) and Sr[j - 1] - Sr[j] < 1e-6 * Sr[j - 1]:
            break                                                  # a cluster cut by K: not determined by either solver
        P = Ur[:, k:j]
        err = np.linalg.norm(got[:, k:j] - P @ (P.T @ got[:, k:j]))
        print(kind, "cluster", k, j, err)
        assert err < 1e-5 * np.sqrt(j - k), (kind, k, j)
        k = j
