"""CPU: the host side of the global step's slab solver -- the NumPy model of tests/gslab_model.py against the
longdouble-refined ``splu`` solution at the shapes tests/test_gpu_gslab.py runs on the device, ``projections.slab_plan`` on the
matrices of the five element kinds, the refusals of ``posSnapshots.set_global_solver`` and the engine calls of the public
methods under "slab" on a recording double.

Bound: 64 eps kappa(A) max |x| (tests/gslab_model.py); the model is held to a TENTH of it.  Observed on this model, error / bound:
chains at most 7e-3, the 6^3 grid 8e-4, the 10^3 grid (wi = 1e3, kappa 57.5) 8e-4, the stiff 8^3 grid (wi = 1e6, kappa 8.5e5) 4e-4."""
import types

import numpy as np
import pytest
from scipy import sparse

from conftest import load_golden
from gslab_model import EPS, bound, chain_matrix, grid_matrix, model_solve, refined_solve, rhs

from animsnapbases_amd import projections as proj

CHAINS = [1, 2, 15, 16, 17, 31, 33, 65]
TARGETS = [1, 4, 16, None]                      # None: one slab


def _held(A, target, w, tag):
    """The model within a tenth of the bound of the refined solution; returns error / bound."""
    n = A.shape[0]
    plan = proj.slab_plan(A, n if target is None else target)
    B = rhs(n, w, 5 * n + w)
    ref = refined_solve(A, B)
    got = model_solve(A, plan, B)
    kappa = np.linalg.cond(A.toarray())
    bnd = bound(kappa, ref)
    err = float(np.abs(got.astype(np.longdouble) - ref).max())
    print("%s target %s: %d slabs, kappa %.3g, err / bound %.3g" % (tag, target, len(plan.slab_ptr) - 1, kappa, err / bnd))
    assert err <= 0.1 * bnd, (tag, target, err, bnd)
    return err / bnd


@pytest.mark.parametrize("n", CHAINS)
def test_model_on_chains(n):
    A = chain_matrix(n)
    for target in TARGETS:
        _held(A, target, 5, "chain %d" % n)


@pytest.mark.parametrize("nx,wi,m0,target", [(6, 1e3, 0.3, 32), (10, 1e3, 0.3, 256), (8, 1e6, 0.02, 64)])
def test_model_on_grids(nx, wi, m0, target):
    A = grid_matrix(nx, wi, m0)
    _held(A, target, 7, "grid %d^3 wi %g" % (nx, wi))
    # the residual of the model's solution, the quantity the device reports for u = 1
    plan = proj.slab_plan(A, target)
    y = model_solve(A, plan, np.ones((A.shape[0], 1)))
    assert np.abs(A @ y - 1.0).max() <= 64 * EPS * np.linalg.cond(A.toarray())


# ------------------------------------------------------------------ slab_plan
def _kind_matrix(name):
    if name == "combined":
        ge, gt = load_golden("cproj_edge_spring"), load_golden("cproj_tets_strain")
        N = gt["rest"].shape[0]
        specs = [(proj.build_setup("edge_spring", ge["elements"], ge["rest"]), 0.7), (proj.build_setup("tets_strain", gt["elements"], gt["rest"]), 0.7)]
    else:
        g = load_golden("cproj_" + name)
        N = g["rest"].shape[0]
        specs = [(proj.build_setup("verts_bending" if name.startswith("verts_bending") else name, g["elements"], g["rest"]), 0.7)]
    return proj.global_matrix(specs, N, 0.5 + np.random.default_rng(2).random(N), 0.5)


def _check_plan(A, plan):
    n = A.shape[0]
    assert sorted(plan.order.tolist()) == list(range(n))
    assert plan.slab_ptr[0] == 0 and plan.slab_ptr[-1] == n and (np.diff(plan.slab_ptr) >= 1).all()
    assert abs(plan.A_perm - A[plan.order][:, plan.order]).max() == 0.0 and plan.A_perm.has_sorted_indices
    slab = np.searchsorted(plan.slab_ptr, np.arange(n), side="right") - 1
    coo = plan.A_perm.tocoo()
    assert (np.abs(slab[coo.row] - slab[coo.col]) <= 1).all()


@pytest.mark.parametrize("name", ["edge_spring", "tris_strain", "tets_strain", "tets_deformation_gradient", "verts_bending_grid",
                                  "verts_bending_closed", "combined"])
def test_slab_plan_on_the_golden_kinds(name):
    A = _kind_matrix(name)
    n = A.shape[0]
    for target in (1, 4, n, 10 * n):
        plan = proj.slab_plan(A, target)
        _check_plan(A, plan)
        if target >= n:
            assert len(plan.slab_ptr) == 2
        # the plan serves the solve: the model on it reproduces the dense solution
        B = rhs(n, 3, n)
        x = model_solve(A, plan, B)
        ref = np.linalg.solve(A.toarray(), B)
        assert np.abs(x - ref).max() <= 64 * EPS * np.linalg.cond(A.toarray()) * np.abs(ref).max()
    assert len(proj.slab_plan(A, 1).slab_ptr) > 3           # several slabs at the small targets the GPU tests set


def test_slab_plan_disconnected_single_vertex_and_one_slab():
    a, b = chain_matrix(17), chain_matrix(5, seed=1)
    A = sparse.block_diag([a, b, sparse.csr_matrix(np.array([[3.0]]))]).tocsr()
    mix = np.random.default_rng(1).permutation(A.shape[0])
    A = A[mix][:, mix].tocsr()
    A.sort_indices()
    for target in (1, 3, 100):
        plan = proj.slab_plan(A, target)
        _check_plan(A, plan)
        B = rhs(A.shape[0], 2, 9)
        assert np.abs(model_solve(A, plan, B) - np.linalg.solve(A.toarray(), B)).max() <= 1e-12 * np.abs(B).max()
    one = proj.slab_plan(sparse.csr_matrix(np.array([[2.5]])), 1536)
    assert one.order.tolist() == [0] and one.slab_ptr.tolist() == [0, 1] and one.A_perm.toarray().tolist() == [[2.5]]
    assert np.array_equal(model_solve(None, one, np.array([[5.0]])), np.array([[2.0]]))
    assert proj.slab_plan(chain_matrix(65), 10 ** 6).slab_ptr.tolist() == [0, 65]


def test_slab_plan_refuses_a_broken_plan():
    A = chain_matrix(33)
    plan = proj.slab_plan(A, 4)
    assert len(plan.slab_ptr) > 4
    proj.check_slab_plan(plan.A_perm, plan.slab_ptr)
    broken = plan.A_perm.tolil()
    broken[0, 32] = broken[32, 0] = -0.125                  # the first slab coupled to the last
    with pytest.raises(ValueError, match="not block tridiagonal"):
        proj.check_slab_plan(broken.tocsr(), plan.slab_ptr)
    for ptr in ([0, 10, 10, 33], [1, 33], [0, 20], [0]):
        with pytest.raises(ValueError, match="do not cover"):
            proj.check_slab_plan(plan.A_perm, np.array(ptr))
    for bad in (0, -3, 2.5, "many", True):
        with pytest.raises(ValueError, match="target"):
            proj.slab_plan(A, bad)
    with pytest.raises(ValueError, match="square"):
        proj.slab_plan(A[:5], 4)


# ------------------------------------------------------------------ the public switch on a recording double
class _Recorder(object):
    """Records the names of the engine methods called; answers what the callers read back."""
    device_id = 0

    def __init__(self):
        self.calls, self.held, self._frames = [], None, None

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*args, **kw):
            self.calls.append(name)
            return getattr(self, "_" + name, lambda *a, **k: None)(*args, **kw)
        return call

    def _gstep_setup(self, A):
        return 0.0

    def _gslab_held(self, A, plan):
        return self.held

    def _gslab_setup(self, A, plan):
        self.plan = plan
        self.held = (0.0, (len(plan.slab_ptr) - 1, 16))
        return self.held

    def _pdsolve_begin(self, which, f0, f1, fj, *rest):
        self._frames = len(range(f0, f1, fj))

    def _pdsolve_iterate(self, n_iter, chunk_frames=0, out_dev_ptr=None, history=False):
        return np.ones((n_iter, self._frames, 2)) if history else None

    def _force_diff(self, a, b, F, N, per_frame=False):
        return np.ones(3), 1.0, np.ones(4), np.ones((F, 2)) if per_frame else None


def _bare(eng):
    from animsnapbases_amd.posSnapshots import posSnapshots
    g = load_golden("cproj_tets_strain")
    frames = np.array(g["frames"])
    snaps = posSnapshots.__new__(posSnapshots)
    snaps._engine, snaps._comm = eng, types.SimpleNamespace(multi=False)
    snaps.frs, snaps.nVerts = frames.shape[:2]
    snaps.verts, snaps.tris, snaps.test_verts, snaps._snapTensor = frames, None, None, None
    snaps.mass = 0.5 + np.random.default_rng(5).random(frames.shape[1])
    snaps.massL = np.sqrt(snaps.mass)
    snaps.invMassL = 1.0 / snaps.massL
    snaps._standarize, snaps.pre_scale_factor = False, 1.0
    snaps.mean = None
    snaps.assembly_ST = snaps.bending_indices = snaps.global_matrix = snaps.global_solve_residual = None
    kind = dict(kind="tets_strain", elements=g["elements"], wi=0.7, rest_positions=g["rest"], sigma_min=float(g["sigma"][0]),
                sigma_max=float(g["sigma"][1]))
    return snaps, kind


def test_set_global_solver_refusals_touch_no_engine():
    eng = _Recorder()
    snaps, kind = _bare(eng)
    for args in (("dense",), (None,), ("slab", 0), ("slab", -4), ("slab", 2.5), ("slab", "big"), ("slab", True), ("inverse", 64)):
        with pytest.raises(ValueError, match="set_global_solver"):
            snaps.set_global_solver(*args)
    assert snaps._slab_solver() is None                         # a refused call changes nothing
    snaps.set_global_solver("slab")
    assert snaps._slab_solver() == proj.SLAB_TARGET == 256
    snaps.set_global_solver("slab", 4)
    assert snaps._slab_solver() == 4
    with pytest.raises(ValueError, match="history"):
        snaps.solve_frames([kind], 0.5, 3, history=True)
    snaps.set_global_solver()
    assert snaps._slab_solver() is None
    assert eng.calls == []


def test_engine_calls_under_slab(monkeypatch):
    import torch
    real = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **kw: real(*a, **kw))
    eng = _Recorder()
    snaps, kind = _bare(eng)
    snaps.set_global_solver("slab", 4)
    solve = ["pdsolve_begin", "cproj_setup", "pdsolve_slot", "pdsolve_iterate"]
    snaps.solve_frames([kind], 0.5, 3)
    assert eng.calls == ["gslab_held", "gslab_setup"] + solve
    assert snaps.global_solve_slabs[0] == len(eng.plan.slab_ptr) - 1 > 2 and snaps.global_solve_slabs[1] == np.diff(eng.plan.slab_ptr).max()
    assert snaps.global_matrix is not None and snaps.global_solve_residual == 0.0
    # the factor the engine holds is kept; no call of the inverse's set-up appears
    del eng.calls[:]
    snaps.simulate_frames([kind], 0.5, 2, 3)
    assert eng.calls == ["gslab_held", "pdsolve_begin", "pdsolve_carry", "cproj_setup", "pdsolve_slot", "pdsolve_iterate", "pdsolve_advance",
                         "pdsolve_iterate", "pdsolve_positions"]
    # back to the default: exactly the calls of the explicit inverse
    del eng.calls[:]
    snaps.set_global_solver("inverse")
    snaps.solve_frames([kind], 0.5, 3)
    assert eng.calls == ["gstep_held", "gstep_setup"] + solve
