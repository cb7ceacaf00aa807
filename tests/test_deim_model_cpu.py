"""CPU: tests/deim_model.py (the longdouble model the GPU tests of the interpolation-point kernels compare with) against the
oracle and the float64 host loop of constraintsComponents.deim(), and the conditions the GPU cases of tests/deim_cases.py
rely on: energy gaps of the DEIM runs, separation of the single steps, bit-identical ties, the shard plan's split form."""
import contextlib
import io
import types

import numpy as np
import pytest

import deim_cases as dc
import deim_model as dm
from oracle import asb_oracle as orc

LD = np.longdouble


class _HostEngine(object):
    """float64 numpy written to the contract of asb_deim_step / asb_deim_row (include/asb.h), one shard"""

    def __init__(self, comps):
        self.comps = np.asarray(comps, dtype=np.float64)

    def deim_step(self, k, coef=None):
        r = -self.comps[k].copy()
        if k:
            r += np.einsum("ij,jei->ei", coef, self.comps[:k])
        e = (r ** 2).sum(axis=1)
        return int(np.argmax(e)), float(e.max())

    def deim_row(self, gidx):
        return self.comps[:, gidx, :].copy()


def host_loop(comps):
    """constraintsComponents.deim() with its host loop (bordered inverse in float64, lstsq as fallback)"""
    from animsnapbases_amd import constraintsComponents
    cc = object.__new__(constraintsComponents)
    cc.nonlinearSnapshots = types.SimpleNamespace(_engine=_HostEngine(comps), _comm=types.SimpleNamespace(multi=False, rank=0),
                                                  constraintsSize=1)
    cc.numComp = comps.shape[0]
    cc._comps_on_device = False
    cc._rank_diagnostic = lambda K: None
    cc.geom_interpol_verts = []
    with contextlib.redirect_stdout(io.StringIO()):
        cc.deim()
    return cc.geom_Pt


@pytest.mark.parametrize("n,K,seed", [(40, 12, 1), (200, 60, 2), (90, 50, 3)])
def test_model_equals_the_oracle_and_the_host_loop(n, K, seed):
    rng = np.random.default_rng(seed)
    comps = np.stack([np.linalg.qr(rng.normal(size=(n, K)))[0].T for _ in range(3)], axis=2)
    m = dm.deim_loop(comps, float64_too=True)
    assert m["gap"].min() > dc.RUN_GAP
    assert m["Pt"].tolist() == orc.deim(comps, 1)["Pt"].tolist()
    assert m["Pt"].tolist() == host_loop(comps).tolist()
    assert len(set(m["Pt"].tolist())) == K
    assert np.max(np.abs(m["maxabs64"] - m["maxabs"]) / m["maxabs"]) < 1e-9        # (float64 against longdouble: sanity only)


def test_both_solvers_of_the_model_agree():
    rng = np.random.default_rng(5)
    for n in (1, 2, 17, 48, 90):
        A, b = rng.normal(size=(n, n)) + 3 * np.eye(n), rng.normal(size=n)
        x, y = dm.gauss_solve(A, b), dm.refined_solve(A, b)
        assert np.abs(x - y).max() <= 1e-16 * np.abs(x).max()
        assert np.abs(A.astype(LD) @ x - b).max() <= 1e-17 * (np.abs(A).sum(axis=1).max() * np.abs(x).max())


@pytest.fixture(scope="module")
def golden_runs():
    return dc.run_golden()


@pytest.mark.parametrize("K", sorted(dc.RUN_SEEDS))
def test_deim_run_cases_keep_the_gap_and_the_golden_table_is_the_models(K, golden_runs):
    """(d): no step of any listed case may have its two best rows closer than RUN_GAP (relative); the committed table
    tests/golden/deim_run_model.npz is what the model computes"""
    m = dm.deim_loop(dc.run_basis(K))
    g = golden_runs[K]
    assert float(m["gap"].min()) > dc.RUN_GAP, (K, float(m["gap"].min()))
    assert m["Pt"].tolist() == g["Pt"].tolist() and len(set(m["Pt"].tolist())) == K
    assert np.max(np.abs(m["maxabs"].astype(np.float64) - g["maxabs"]) / g["maxabs"]) < 1e-15
    assert np.allclose(m["gap"].astype(np.float64), g["gap"], rtol=1e-9, atol=0)
    assert 0 <= g["dev64"] < 1e-8                      # (the recorded measurement: the GPU tolerance is 16 times it)


@pytest.mark.parametrize("n,K,k,v0,N", dc.STEP_CASES)
def test_step_cases_are_separated(n, K, k, v0, N):
    """(a): best and second-best energy of every listed case differ by more than the bound of either"""
    comps, coef = dc.step_inputs(n, K, k)
    s = dm.step(comps, k, coef)
    assert s["ebound"].max() < 1e-9 * float(s["val"])
    if n > 1:
        assert float(s["val"] - s["second"]) > 2 * s["ebound"].max()


@pytest.mark.parametrize("name,n,rows", dc.TIE_CASES)
def test_tie_generators_give_bit_identical_maxima(name, n, rows):
    comps = dc.tie_basis(n, rows)
    for k, coef in ((0, None), (1, np.full((3, 1), 0.5))):
        r = -comps[k].copy()
        if k:
            r += coef[:, 0][None, :] * comps[0]                    # float64, the kernel's operations
        e = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]
        top = np.flatnonzero(e == e.max())
        assert top.tolist() == sorted(rows), (name, k)
        assert dm.step(comps, k, coef)["idx"] == min(rows)
    for p in (1, 2):
        if n * p > 2 * dc.BIG_N:
            continue
        blk = dc.tie_block_basis(n, p, rows)
        e = (blk ** 2).sum(axis=(0, 2))
        assert np.flatnonzero(e == e.max()).tolist() == sorted(c * p + q for c in rows for q in range(p))
        ec = e.reshape(n, p).sum(axis=1)
        assert np.flatnonzero(ec == ec.max()).tolist() == sorted(rows)


def test_st_tie_rows_are_identical():
    St = dc.st_tie(dc.st_matrix(1000, dc.ST_COLS, 3, long_row=False), (100, 700))
    a, b = St[100], St[700]
    assert np.array_equal(a.indices, b.indices) and np.array_equal(a.data, b.data) and a.nnz == 5


@pytest.mark.parametrize("world", [1, 2, 3])
def test_shard_plan_through_the_split_form_equals_the_unsplit_form(world):
    from animsnapbases_amd.constraints import st_shard_plan
    from animsnapbases_amd.distributed import partition
    St = dc.st_matrix(200, 97, 11)
    M = np.random.default_rng(4).normal(size=(97, 10))
    whole = dm.st_rows(St.indptr, St.indices, St.data, M)
    assert np.all(whole["energy"][np.diff(St.indptr) == 0] == 0)
    shards = partition(97, world)
    seen = np.zeros(200, dtype=int)
    for r in range(world):
        pl = st_shard_plan(St, shards, r)
        v0, n = shards[r]
        part = dm.st_rows_split(pl["indptr"], pl["slots"], pl["data"], M[v0:v0 + n], M[pl["halo"]])
        assert np.array_equal(part["energy"], whole["energy"][pl["owned"]])             # same terms in the same order
        assert np.array_equal(part["amax"], whole["amax"][pl["owned"]])
        seen[pl["owned"]] += 1
    assert np.all(seen == 1)


def test_model_rows_of_a_small_matrix_by_hand():
    indptr, indices, data = np.array([0, 2, 2, 3]), np.array([0, 2, 1]), np.array([2.0, -1.0, 0.5])
    M = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
    s = dm.st_rows(indptr, indices, data, M)
    assert s["acc"].tolist() == [[-3.0, -2.0], [0.0, 0.0], [1.5, 2.0]]
    assert s["energy"].tolist() == [13.0, 0.0, 6.25] and s["amax"].tolist() == [3.0, 0.0, 2.0]
    b = dm.block_step(np.arange(24.0).reshape(4, 2, 3), 1, 2, np.ones((3, 2, 2)), 2)
    # r[e, m, i] = V[e,0,i] + V[e,1,i] - V[e,2+m,i]
    assert b["r"][1, 1].tolist() == [3 + 9 - 21.0, 4 + 10 - 22.0, 5 + 11 - 23.0]
