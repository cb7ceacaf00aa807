"""CPU: tests/pod_model.py against LAPACK -- CholeskyQR against scipy's economic QR, the one-sided Jacobi against numpy's SVD, the
chain basis -> CholeskyQR2 -> project -> rotate against the SVD of the snapshots, the power step and the deflation on exact
singular vectors -- and the longdouble model against the float64 model at the shapes tests/test_gpu_pod_phases.py uses: the
device tolerances there are multiples of that deviation."""
import numpy as np
import pytest
import scipy.linalg

import pod_model as pm
import test_gpu_pod_phases as gp

LD = np.longdouble
EPS = 2.0 ** -52


def _orthonormal(rng, rows, cols):
    return np.linalg.qr(rng.normal(size=(rows, cols)))[0]


def _snapshots(rng, F, n, s):
    """(F, n, 3) whose matrix A (3 n, F) has the singular values s, with its factors"""
    U, V = _orthonormal(rng, 3 * n, len(s)), _orthonormal(rng, F, len(s))
    return pm.unrows((U * s[None]) @ V.T, n), U, V


@pytest.mark.parametrize("dtype", (np.float64, LD))
@pytest.mark.parametrize("K", (1, 5, 64))
def test_chol_qr_is_the_economic_qr(K, dtype):
    rng = np.random.default_rng(K)
    n = 2 * K + 1
    C = rng.normal(size=(K, n, 3))
    per_slice = pm.chol_qr(C, pm.slice_grams(C, dtype), False, dtype)
    joint = pm.chol_qr(C, pm.slice_grams(C, dtype), True, dtype)
    assert per_slice.dtype == dtype and joint.dtype == dtype
    for l in range(3):
        Q = scipy.linalg.qr(C[:, :, l].T, mode="economic")[0].T
        assert pm.deviation(pm.align_signs(per_slice[:, :, l].astype(np.float64), Q), Q)[1] < 1e-13
    Q = scipy.linalg.qr(pm.flat(C).T, mode="economic")[0].T
    assert pm.deviation(pm.align_signs(pm.flat(joint).astype(np.float64), Q), Q)[1] < 1e-13
    assert max(pm.orth_defect(per_slice, False)) < 1e-13 and max(pm.orth_defect(joint, True)) < 1e-13
    assert pm.deviation(pm.joint_gram(C, dtype), pm.flat(C, LD) @ pm.flat(C, LD).T)[1] < 10 * EPS


def test_chol_qr_refuses_a_pivot_that_is_not_positive():
    rng = np.random.default_rng(1)
    C = rng.normal(size=(4, 9, 3))
    C[2] = 0.0
    for joint in (False, True):
        with pytest.raises(ValueError, match="rank deficient: pivot 2"):
            pm.chol_qr(C, pm.slice_grams(C), joint)
    C[2] = C[0] + C[1]              # dependent, pivot at rounding level with either sign: a refusal or a huge factor
    G = pm.slice_grams(C, LD)
    try:
        assert np.abs(pm.chol_qr(C, G, True, LD)).max() > 1e6
    except ValueError:
        pass


@pytest.mark.parametrize("dtype", (np.float64, LD))
@pytest.mark.parametrize("K", (1, 2, 5, 64))
def test_rotate_is_the_svd(K, dtype):
    rng = np.random.default_rng(10 + K)
    F, n = K + 6, K + 1
    s = np.geomspace(1.0, 1e-2, K)
    B = gp._prescribed_b(rng, K, F, s)
    Q = _orthonormal(rng, 3 * n, K).T.reshape(K, n, 3)
    S, U, R, Cn = pm.rotate(Q, B, dtype)
    assert all(a.dtype == dtype for a in (S, U, R, Cn))
    Ul, Sl, Vt = np.linalg.svd(B, full_matrices=False)
    assert np.abs(S.astype(np.float64) - Sl).max() < 1e-13 and np.abs(Sl - s).max() < 1e-13
    assert (S[:-1] > S[1:]).all() or K == 1
    # the gaps are >= 3.6 % of s: every vector is determined to ~ eps / gap
    assert pm.deviation(pm.align_signs(U.astype(np.float64), Ul.T), Ul.T)[1] < 1e-11
    assert pm.deviation(pm.align_signs(R.astype(np.float64), Sl[:, None] * Vt), Sl[:, None] * Vt)[1] < 1e-11
    assert pm.deviation(U @ np.asarray(B, dtype=dtype), R)[1] < 1e-13
    assert pm.deviation(Cn, (U @ pm.flat(Q, dtype)).reshape(K, n, 3))[1] == 0.0
    assert max(pm.orth_defect(Cn, True)) < 1e-12


def test_jacobi_keeps_a_zero_row():
    rng = np.random.default_rng(3)
    B = np.insert(gp._prescribed_b(rng, 5, 9, np.geomspace(1.0, 1e-2, 5)), 2, 0.0, axis=0)
    S, U, R, _ = pm.rotate(np.zeros((6, 2, 3)), B, LD)
    assert S[-1] == 0 and (R[-1] == 0).all() and U[-1].tolist() == [0, 0, 1, 0, 0, 0]


@pytest.mark.parametrize("dtype", (np.float64, LD))
def test_the_chain_reproduces_the_svd(dtype):
    """basis from the Gram matrix's eigen-pairs, CholeskyQR2, project, rotate: the singular values and left vectors of A"""
    rng = np.random.default_rng(20)
    F, n, K = 12, 10, 6
    s = np.geomspace(1.0, 1e-3, F)
    X, U, V = _snapshots(rng, F, n, s)
    A = pm.rows(X)
    lam, W = np.linalg.eigh(A.T @ A)
    lam, W = lam[::-1], W[:, ::-1]
    C = pm.basis(X, W, lam, K, dtype)
    for _ in range(2):
        C = pm.chol_qr(C, pm.slice_grams(C, dtype), True, dtype)
    B = pm.project(C, X, dtype)
    S, _, R, Cn = pm.rotate(C, B, dtype)
    Ul, Sl, Vt = np.linalg.svd(A, full_matrices=False)
    assert np.abs(S.astype(np.float64) - Sl[:K]).max() < 1e-13
    got = pm.flat(Cn).astype(np.float64)
    assert pm.deviation(pm.align_signs(got, Ul[:, :K].T), Ul[:, :K].T)[1] < 1e-10       # (eps sigma_0^2 / sigma_K^2 / gap)
    assert max(pm.orth_defect(Cn, True)) < 1e-13


@pytest.mark.parametrize("dtype", (np.float64, LD))
def test_power_keeps_an_exact_singular_basis(dtype):
    rng = np.random.default_rng(30)
    F, n, K = 10, 6, 4
    s = np.geomspace(1.0, 1e-2, F)
    X, U, V = _snapshots(rng, F, n, s)
    C = U[:, :K].T.reshape(K, n, 3)
    B_rot = s[:K, None] * V[:, :K].T
    P = pm.power(X, B_rot, s[:K], dtype)
    assert P.dtype == dtype and pm.deviation(P, C)[1] < 1e-13
    S0 = s[:K].copy()
    S0[2] = 0.0
    P0 = pm.power(X, B_rot, S0, dtype)
    assert (P0[2] == 0).all() and np.array_equal(np.delete(P0, 2, axis=0), np.delete(P, 2, axis=0))


@pytest.mark.parametrize("dtype", (np.float64, LD))
def test_deflate_removes_the_kept_singular_values(dtype):
    rng = np.random.default_rng(40)
    F, n, keep = 8, 6, 2
    s = np.concatenate([[1.0, 0.7], np.geomspace(2e-3, 5e-4, F - 2)])
    X, U, V = _snapshots(rng, F, n, s)
    D = pm.deflate(X, U[:, :keep].T.reshape(keep, n, 3), s[:keep, None] * V[:, :keep].T, dtype)
    assert D.dtype == dtype and D.shape == X.shape
    left = np.linalg.svd(pm.rows(D).astype(np.float64), compute_uv=False)
    assert np.abs(left[:F - keep] - s[keep:]).max() < 1e-15 and left[F - keep:].max() < 1e-15


def test_element_wise_phases():
    rng = np.random.default_rng(50)
    X, C = rng.normal(size=(4, 5, 3)), rng.normal(size=(2, 5, 3))
    mean, w = rng.normal(size=(5, 3)), rng.uniform(0.5, 2, size=5)
    Y = pm.affine(X, 0.3, mean, w)
    assert Y[2, 3, 1] == (X[2, 3, 1] * 0.3 + mean[3, 1]) * w[3]
    assert np.array_equal(pm.affine(X, 1.0, None, None), X)
    assert pm.affine_terms(X, 0.3, mean, w)[2, 3, 1] == (abs(LD(X[2, 3, 1]) * LD(0.3)) + abs(LD(mean[3, 1]))) * LD(w[3])
    Z = pm.comps_post(C, True, 3.7, mean, w)
    assert Z[1, 4, 2] == (C[1, 4, 2] / 3.7 + mean[4, 2]) * w[4]
    assert np.array_equal(pm.comps_post(C, False, 3.7, mean, None), C)
    assert pm.affine(X, 0.3, mean, w, LD).dtype == LD and pm.comps_post(C, True, 3.7, mean, w, LD).dtype == LD
    assert np.array_equal(pm.unrows(pm.rows(X), 5), X)


# ------------------------------------------------------------------------------------------------ longdouble against float64
def _agree(name, lo, hi, bound, worst):
    fro, mx = pm.deviation(lo, hi)
    worst[name] = max(worst.get(name, 0.0), fro, mx)
    assert max(fro, mx) <= bound, (name, fro, mx, bound)
    assert gp.MARGIN * max(fro, mx) <= gp.CEIL, (name, "the device bound would be above the ceiling")


def test_longdouble_and_float64_models_agree_at_the_gpu_shapes():
    """a few eps in the products, below 1e-14 after a CholeskyQR pass (cond ~ 5), below 2e-13 after the Jacobi sweeps
    (K = 128: ~ 10 sweeps of 127 rotations per row)"""
    worst = {}
    rng = np.random.default_rng(60)
    for K in gp.GRAM_K:
        C = rng.normal(size=(K, max(gp.GRAM_N), 3))
        _agree("orth_gram", pm.slice_grams(C), pm.slice_grams(C, LD), 20 * EPS, worst)
    for K in gp.QR_K:
        for n in (2 * K + 1, 2 * K + 2, K):
            C = rng.normal(size=(K, n, 3))
            G = pm.slice_grams(C)
            for joint in (False, True):
                if n == K and not (joint and K % 2 == 0):
                    continue
                _agree("chol_qr", pm.chol_qr(C, G, joint), pm.chol_qr(C, G, joint, LD), 1e-14 if n > K else 1e-12, worst)
    for F in gp.BASIS_F:
        X = gp._low_rank_plus_noise(rng, F, max(gp.BASIS_N))
        A = pm.rows(X)
        lam, V = np.linalg.eigh(A.T @ A)
        K = min(max(gp.BASIS_K), F)
        _agree("basis", pm.basis(X, V[:, ::-1], lam[::-1], K), pm.basis(X, V[:, ::-1], lam[::-1], K, LD), 50 * EPS, worst)
    for K in gp.PROJ_K:
        X, C = rng.normal(size=(max(gp.PROJ_F), max(gp.PROJ_N), 3)), rng.normal(size=(K, max(gp.PROJ_N), 3))
        _agree("project", pm.project(C, X), pm.project(C, X, LD), 20 * EPS, worst)
    for K in gp.ROT_K:
        F, n = K + 6, K + 2
        B = gp._prescribed_b(rng, K, F, np.geomspace(1.0, 1e-2, K))
        Q = _orthonormal(rng, 3 * n, K).T.reshape(K, n, 3)
        lo, hi = pm.rotate(Q, B), pm.rotate(Q, B, LD)
        for name, a, b in zip(("S", "U", "rows", "basis"), lo, hi):
            _agree("rotate " + name, a if name == "S" else pm.align_signs(a, b), b, 2e-13, worst)
        if K in gp.POWER_K:
            X = rng.normal(size=(F, n, 3))
            _agree("power", pm.power(X, hi[2].astype(np.float64), hi[0].astype(np.float64)),
                   pm.power(X, hi[2].astype(np.float64), hi[0].astype(np.float64), LD), 50 * EPS, worst)
    for F, n, K1, _ in gp.DEFLATE_SHAPES:
        X = gp._two_groups(rng, F, n)
        C = _orthonormal(rng, 3 * n, K1).T.reshape(K1, n, 3)
        B = pm.project(C, X)
        _agree("deflate", pm.deflate(X, C[:2], B[:2]), pm.deflate(X, C[:2], B[:2], LD), 20 * EPS, worst)
    print({k: "%.1e" % v for k, v in worst.items()})


def test_the_gpu_case_tables_cover_the_edges():
    """the closing test of the GPU module needs no GPU: it is run here as well"""
    gp.test_cases_cover_the_edges()
