"""CPU: the host side of the global step in a position subspace -- ``projections.subspace_basis``, the refusals of
``posSnapshots.set_global_solver``, the engine calls of the public methods under "subspace" on a recording double, the defining
properties of the longdouble model of tests/gsub_model.py, and the facts about the fixtures that tests/gsub_cases.py relies on
(full rank, amplification, the r = N model against the full one, the non-vacuity margin of r in {4, 8})."""
import types

import numpy as np
import pytest

from conftest import load_golden
from gslab_model import chain_matrix
from gsub_cases import RANKS, amps, apply_bound, residual_bound, sub_case
from gsub_model import EPS, Galerkin, svd_basis, vertex_major
import pdsolve_cases as pc

from animsnapbases_amd import projections as proj


# ------------------------------------------------------------------ subspace_basis
def test_subspace_basis_spans_what_the_basis_spans_and_leaves_its_input(tmp_path):
    rng = np.random.default_rng(3)
    K, N = 7, 23
    comps = rng.standard_normal((K, N, 3)) * 10.0 ** rng.integers(-3, 4, size=(K, 1, 1))       # scale does not matter
    keep = comps.copy()
    for r in (1, 4, None):
        Qt = proj.subspace_basis(comps, r, N)
        k = K if r is None else r
        assert Qt.shape == (3, k, N) and Qt.dtype == np.float64 and Qt.flags["C_CONTIGUOUS"]
        for d in range(3):
            U = comps[:k, :, d].T
            assert np.abs(Qt[d] @ Qt[d].T - np.eye(k)).max() <= 16 * EPS
            assert np.abs(Qt[d].T @ (Qt[d] @ U) - U).max() <= 64 * EPS * np.abs(U).max()       # U lies in span(Q)
    assert np.array_equal(comps, keep)
    # a path and a posComponents: its comps times its snapshots' invMassL (not where q_massWeight has done that already)
    path = tmp_path / "basis.npy"
    np.save(path, comps)
    assert np.array_equal(proj.subspace_basis(str(path), 4), proj.subspace_basis(comps, 4))
    assert np.array_equal(proj.subspace_basis(path, 4), proj.subspace_basis(comps, 4))
    inv = 1.0 / np.sqrt(0.5 + rng.random(N))
    # a posComponents of the package's own class (no engine: its attributes are set by hand, its ``comps`` property is the class's)
    import inspect
    from animsnapbases_amd.posComponents import posComponents
    init = inspect.getsource(posComponents.__init__)
    assert all(name in init for name in ("self.pos_snapshots", "self.param", "self._comps_post_processed")) and isinstance(posComponents.comps, property)
    pcomp = posComponents.__new__(posComponents)
    pcomp._comps, pcomp._comps_on_device, pcomp._comps_post_processed = comps, False, False
    pcomp.pos_snapshots, pcomp.param = types.SimpleNamespace(invMassL=inv), types.SimpleNamespace(q_massWeight=False)
    weighted = proj.subspace_basis(comps * inv[None, :, None], 4)
    assert np.array_equal(proj.subspace_basis(pcomp, 4), weighted)
    pcomp.param.q_massWeight = True                             # asked for, but post_process_components has not run: still weighted
    assert np.array_equal(proj.subspace_basis(pcomp, 4), weighted)
    pcomp._comps_post_processed = True                          # it has run: the comps are in world space already
    assert np.array_equal(proj.subspace_basis(pcomp, 4), proj.subspace_basis(comps, 4))
    pcomp.param.q_massWeight = False                            # post-processed without the mass step: still weighted
    assert np.array_equal(proj.subspace_basis(pcomp, 4), weighted)
    pcomp.pos_snapshots.invMassL = None                         # snapshots without masses: nothing to undo
    assert np.array_equal(proj.subspace_basis(pcomp), proj.subspace_basis(comps))
    assert np.array_equal(comps, keep)


def test_subspace_basis_refusals():
    rng = np.random.default_rng(4)
    comps = rng.standard_normal((6, 9, 3))
    for d, name in enumerate("xyz"):
        bad = comps.copy()
        bad[3, :, d] = 2.0 * bad[1, :, d] - bad[0, :, d]
        with pytest.raises(ValueError, match="rank deficient in coordinate %s" % name):
            proj.subspace_basis(bad)
        assert proj.subspace_basis(bad, 3).shape == (3, 3, 9)       # the first three are independent
    with pytest.raises(ValueError, match="rank deficient"):
        proj.subspace_basis(np.zeros((2, 9, 3)))
    for r in (0, -1, 7, 2.5, "4", True):
        with pytest.raises(ValueError, match="num_components"):
            proj.subspace_basis(comps, r)
    with pytest.raises(ValueError, match="at most N"):
        proj.subspace_basis(rng.standard_normal((5, 4, 3)))
    with pytest.raises(ValueError, match="vertices"):
        proj.subspace_basis(comps, 2, 10)
    for shape in ((6, 9), (6, 9, 2), (0, 9, 3), (6, 0, 3)):
        with pytest.raises(ValueError, match="expected"):
            proj.subspace_basis(np.zeros(shape))
    for v in (np.nan, np.inf):
        bad = comps.copy()
        bad[1, 2, 0] = v
        with pytest.raises(ValueError, match="not finite"):
            proj.subspace_basis(bad)
        assert proj.subspace_basis(bad, 1).shape == (3, 1, 9)       # (only the components in use are judged)
    with pytest.raises(ValueError, match="numeric"):
        proj.subspace_basis([["a"]])


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

    def _gsub_held(self, A, Qt, origin):
        same = self.held is not None and all(np.array_equal(a, b) for a, b in zip(self.held, (A.data, Qt, origin)))
        return 0.25 if same else None

    def _gsub_setup(self, A, Qt, origin):
        self.held = (A.data.copy(), Qt.copy(), origin.copy())
        return 0.25

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
    return snaps, kind, svd_basis(frames)


def test_set_global_solver_refusals_touch_no_engine():
    eng = _Recorder()
    snaps, kind, comps = _bare(eng)
    N = snaps.nVerts
    dep = comps.copy()
    dep[2, :, 2] = dep[0, :, 2]
    bad = [dict(kind="subspace"), dict(kind="subspace", basis=comps[:, :5]), dict(kind="subspace", basis=comps, num_components=0),
           dict(kind="subspace", basis=comps, num_components=N + 1), dict(kind="subspace", basis=dep),
           dict(kind="subspace", basis=comps, origin=np.zeros((N, 2))), dict(kind="subspace", basis=comps, origin=np.full((N, 3), np.nan)),
           dict(kind="subspace", basis=comps, slab_target=4), dict(kind="subspace", basis="no/such/file.npy"),
           dict(kind="inverse", basis=comps), dict(kind="slab", num_components=3), dict(kind="inverse", origin=np.zeros((N, 3))),
           dict(kind="subspaces", basis=comps)]
    for kw in bad:
        with pytest.raises(ValueError, match="set_global_solver"):
            snaps.set_global_solver(**kw)
    with pytest.raises(ValueError, match="rank deficient in coordinate z"):
        snaps.set_global_solver("subspace", basis=dep)
    assert snaps._subspace_solver() is None and snaps._slab_solver() is None                # a refused call changes nothing
    # what exists today keeps its result and its message
    with pytest.raises(ValueError, match="kind must be 'inverse' or 'slab', not 'dense' .or 'subspace'"):
        snaps.set_global_solver("dense")
    with pytest.raises(ValueError, match="slab_target is for kind='slab' only"):
        snaps.set_global_solver("inverse", 64)
    snaps.set_global_solver("slab", 4)
    assert snaps._slab_solver() == 4 and snaps._subspace_solver() is None
    snaps.set_global_solver("subspace", basis=comps, num_components=4)
    Qt, origin = snaps._subspace_solver()
    assert Qt.shape == (3, 4, N) and origin is None and snaps._slab_solver() is None
    with pytest.raises(ValueError, match="history"):
        snaps.solve_frames([kind], 0.5, 3, history=True)
    with pytest.raises(ValueError, match="subspace_solve_errors"):
        snaps.subspace_solve_errors([kind], comps, [4], 0.5)
    snaps.set_global_solver()
    assert snaps._subspace_solver() is None and snaps._slab_solver() is None
    with pytest.raises(ValueError, match="rank deficient"):
        snaps.subspace_solve_errors([kind], dep, [2, 4], 0.5)
    for bad in (2.5, True, 0, "4"):                             # r goes through unchanged: what set_global_solver refuses is refused
        with pytest.raises(ValueError, match="num_components"):
            snaps.subspace_solve_errors([kind], comps, [4, bad], 0.5)
    assert eng.calls == []


def test_engine_calls_under_subspace(monkeypatch):
    import torch
    real = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **kw: real(*a, **kw))
    eng = _Recorder()
    snaps, kind, comps = _bare(eng)
    snaps.set_global_solver("subspace", basis=comps, num_components=4)
    solve = ["pdsolve_begin", "cproj_setup", "pdsolve_slot", "pdsolve_iterate"]
    snaps.solve_frames([kind], 0.5, 3)
    assert eng.calls == ["gsub_held", "gsub_setup"] + solve
    assert snaps.global_solve_subspace == 4 and snaps.global_matrix is not None and snaps.global_solve_residual == 0.25
    assert np.array_equal(eng.held[2], snaps.verts[0])                  # origin None: the rest positions, resolved at the set-up
    # a repeat is held; so is a roll-out
    del eng.calls[:]
    snaps.solve_frames([kind], 0.5, 3)
    assert eng.calls == ["gsub_held"] + solve
    del eng.calls[:]
    snaps.simulate_frames([kind], 0.5, 2, 3)
    assert eng.calls == ["gsub_held", "pdsolve_begin", "pdsolve_carry", "cproj_setup", "pdsolve_slot", "pdsolve_iterate", "pdsolve_advance",
                         "pdsolve_iterate", "pdsolve_positions"]
    # another rank or origin is another set-up
    del eng.calls[:]
    snaps.set_global_solver("subspace", basis=comps, num_components=4, origin=snaps.verts[1])
    snaps.global_solve_setup([kind], 0.5)
    assert eng.calls == ["gsub_held", "gsub_setup"]
    # hyper: the operators behind the matrix, then the affine iteration
    c = __import__("reduced_forces_cases").case("tets_deim")
    spec = dict(kind, basis=c.basis, num_components=c.ms[0], reduction=c.reduction)
    del eng.calls[:]
    snaps.solve_frames([spec], 0.5, 3, hyper="touched")
    assert eng.calls == ["gsub_held", "rforce_operator", "hyper_operator", "pdsolve_begin", "cproj_setup", "rforce_solver", "pdsolve_slot",
                         "hyper_iterate"]
    # the sweep: the full solve under the selected solver, one subspace solve per r, the selection restored
    snaps.set_global_solver("inverse")
    del eng.calls[:]
    out = snaps.subspace_solve_errors([kind], comps, [4, 8], 0.5, 3, per_frame=True)
    assert eng.calls == ["gstep_held", "gstep_setup"] + solve + (["gsub_held", "gsub_setup"] + solve + ["force_diff"]) * 2
    assert len(out) == 6 and out[5].shape[0] == 2 and snaps._subspace_solver() is None and snaps._global_solver == ("inverse", None)
    assert snaps.subspace_solve_errors([kind], comps, [], 0.5, 3) == ([], [], [], [], [])
    # back to the default: exactly the calls of the explicit inverse
    del eng.calls[:]
    snaps.solve_frames([kind], 0.5, 3)
    assert eng.calls == ["gstep_held", "gstep_setup"] + solve


# ------------------------------------------------------------------ the host model
@pytest.mark.parametrize("n", [2, 17, 33, 65])
def test_model_satisfies_the_defining_properties(n):
    rng = np.random.default_rng(40 + n)
    A = chain_matrix(n)
    origin = rng.standard_normal((n, 3))
    for r in sorted(set([1, min(n, 4), n])):
        Qt = proj.subspace_basis(rng.standard_normal((r, n, 3)))
        g = Galerkin(A, Qt, origin)
        R = rng.standard_normal((3 * n, 5))
        for affine in (True, False):
            Q = g.apply(R, affine)
            one = apply_bound(g, R, affine)
            assert one < 1e-10 * max(1.0, np.abs(R).max())
            assert g.residual(Q, R) <= residual_bound(g, one)                       # U^T (A q - rhs) = 0 to rounding
        # rhs = A (o + U z*) returns o + U z*
        z = rng.standard_normal((3, r))
        q = np.stack([origin[:, d] + Qt[d].T @ z[d] for d in range(3)], axis=1)
        assert np.abs(g.solve(A @ q) - q).max() <= apply_bound(g, vertex_major((A @ q)[None]), True)
        if r == n:                                                                  # the full basis: the Galerkin step is A^-1
            b = rng.standard_normal((n, 3))
            ref = np.linalg.solve(A.toarray(), b)
            assert np.abs(g.solve(b) - ref).max() <= 64 * EPS * np.linalg.cond(A.toarray()) * np.abs(ref).max()


@pytest.mark.parametrize("name", pc.NAMES)
def test_the_fixtures_are_suitable(name):
    """What tests/gsub_cases.py states about the cases, on this model: full rank, amp far below AMP_CAP, r = N equals the full
    model, r in {4, 8} differs from it by far more than any bound."""
    c = pc.host_case(name)
    frames = c["frames"]
    F, N = frames.shape[:2]
    for d in range(3):
        assert np.linalg.matrix_rank(frames[:, :, d] - frames[0, :, d][None]) == N
    full = pc.model(c, range(F), "difference", pc.KS)
    for r in RANKS + (None,):
        s = sub_case(name, r)
        assert s["r"] == (N if r is None else r) and max(s["galerkin"].kappa) <= np.linalg.cond(c["A"].toarray()) * (1 + 1e-12)
        for mode in pc.MODES:
            amp = amps(s, mode)
            assert max(amp.values()) < 8.0, (name, r, mode, amp)
        got = pc.model(s, range(F), "difference", pc.KS)
        diff = float(np.abs(got[10] - full[10]).max())
        print("%s r = %s: |model - full| after 10 iterations %.3g" % (name, r, diff))
        if r is None:
            assert max(float(np.abs(got[K] - full[K]).max()) for K in pc.KS) <= 4e-15 * max(1.0, np.abs(full[10]).max())
        else:
            assert 0.05 <= diff <= 1.5
