"""CPU: tests/splocs_model.py -- the per-phase model the GPU tests of the SPLOCS kernels compare with -- is the reference's
algorithm: its float64 phases, chained over three outer iterations, reproduce oracle.asb_oracle.splocs_glob_optimization
(which forms the residual and solves with LAPACK's Cholesky) in C, W, U, Lambda, the centres and the trace, to the tolerance of
the oracle-vs-golden test; the longdouble phases stay in their type and agree with the float64 ones to rounding."""
import numpy as np
import pytest

import splocs_model as sm
from conftest import relerr
from oracle import asb_oracle as orc

K, F, ITS, ADMM_ITS = 6, 30, 3, 5
DMIN, DMAX, LAM, RHO = 0.1, 0.4, 2.0, 10.0


@pytest.fixture(scope="module")
def case():
    rest, tris = orc.synth_mesh(8, 10, seed=3)
    verts = orc.synth_snapshots(rest, F, rank=8, seed=3, kind="bumps")
    X = orc.prepare_snapshots(verts, "first", True)["snapTensor"]
    geo = orc.Geodesics(verts[0], tris)
    d = orc.extract_k_components(X, K, "local", geo, DMIN, DMAX)
    ref = orc.splocs_glob_optimization(X, d["comps"], d["weigs"], d["R"], geo, DMIN, DMAX, ITS, ADMM_ITS, LAM, RHO)
    return X, geo, d, ref


def chain(X, geo, comps, weigs, dtype):
    """the outer loop of posComponents._splocs_glob_optimization on the model's phases"""
    N = X.shape[1]
    C, W, U = np.array(comps, dtype=dtype), np.array(weigs, dtype=dtype), np.zeros(comps.shape, dtype=dtype)
    P, M, nx = sm.gram(X, C, dtype)
    cen, trace = [], []
    for _ in range(ITS):
        W = sm.weights(W, P, M, dtype)
        idx, _ = sm.centres(C, 0, dtype)
        Lambda = sm.lambda_from_fields(np.stack([geo(int(i)) for i in idx]), LAM, DMIN, DMAX, dtype)
        a = sm.admm(X, W, C, U, Lambda, RHO, ADMM_ITS, dtype)
        C, U = a["C"], a["U"]
        P, M, _ = sm.gram(X, C, dtype)
        wp, gm, sp = sm.objective(W, a["G"], P, M, Lambda, C, dtype)
        r2 = nx - 2 * wp + gm
        trace.append([r2 + sp, np.sqrt(r2) / np.sqrt(dtype(3 * N * F))])
        cen.append(idx)
    for v in (C, W, U, Lambda, a["Ginv"], a["c"], P, M):
        assert v.dtype == dtype
    return dict(C=C, W=W, U=U, Lambda=Lambda, idx=np.array(cen), trace=np.array(trace, dtype=dtype))


def test_float64_phases_reproduce_the_oracle(case):
    X, geo, d, ref = case
    got = chain(X, geo, d["comps"], d["weigs"], np.float64)
    assert got["idx"].tolist() == ref["idx"].tolist()
    for name in ("C", "W", "U", "Lambda", "trace"):
        assert relerr(got[name], ref[name]) < 1e-10, (name, relerr(got[name], ref[name]))
    assert np.abs(ref["U"]).max() > 0 and (ref["W"].max(axis=0) == 1).all()        # the case exercises U and the projection


def test_longdouble_phases_stay_in_their_type_and_agree(case):
    X, geo, d, ref = case
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "numpy.longdouble is no wider than float64 here: no high-precision model"
    lo = chain(X, geo, d["comps"], d["weigs"], np.float64)
    hi = chain(X, geo, d["comps"], d["weigs"], np.longdouble)
    assert hi["idx"].tolist() == lo["idx"].tolist()
    for name in ("C", "W", "U", "Lambda", "trace"):
        fro, mx = sm.deviation(lo[name], hi[name])
        assert fro < 1e-11 and mx < 1e-11, (name, fro, mx)


def test_dead_and_all_negative_columns():
    """a column with M[k, k] <= 1e-8 becomes zero; a column whose optimum is <= 0 everywhere becomes zero without a division"""
    rng = np.random.default_rng(0)
    W = rng.uniform(0, 1, size=(9, 4))
    C = rng.normal(size=(4, 5, 3))
    C[1] = 0
    C[3] *= np.sqrt(1e-9 / (C[3] ** 2).sum())
    X = rng.normal(size=(9, 5, 3))
    for dtype in (np.float64, np.longdouble):
        P, M, _ = sm.gram(X, C, dtype)
        P[:, 2] = -100
        out = sm.weights(W, P, M, dtype)
        assert (out[:, [1, 2, 3]] == 0).all() and out[:, 0].max() == 1 and out.min() >= 0 and np.isfinite(out).all()


def test_prox_convention_and_cholesky_inverse():
    for dtype in (np.float64, np.longdouble):
        x = np.zeros((2, 3, 3), dtype=dtype)
        x[0, 1] = [3, 4, 0]
        Lam = np.array([[0, 2.5, 1], [1, 0, 0]], dtype=dtype)
        z = sm.prox_l1l2(Lam, x, dtype(1))
        assert np.isfinite(z).all() and z.dtype == dtype
        assert np.array_equal(z[0, 1], np.array([1.5, 2, 0], dtype=dtype)) and (z[1] == 0).all() and (z[0, [0, 2]] == 0).all()
        rng = np.random.default_rng(1)
        B = rng.normal(size=(17, 9)).astype(dtype)
        A = B @ B.T + dtype(3) * np.eye(17, dtype=dtype)
        Ai = sm.cholesky_inverse(A)
        assert Ai.dtype == dtype
        assert np.abs(Ai @ A - np.eye(17)).max() < 200 * np.finfo(dtype).eps * float(np.linalg.cond(A.astype(np.float64)))
    c, v = sm.centres(np.array([[[0, 0, 5.0], [3, 4, 0], [5, 0, 0]], [[1, 0, 0], [0, 0, 2.0], [0, 2, 0]]]), v0=7)
    assert c.tolist() == [7, 8] and v.tolist() == [25.0, 4.0]
