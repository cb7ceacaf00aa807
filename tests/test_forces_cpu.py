"""CPU: the fixtures of tools/gen_golden_forces.py -- the positions after T time steps of the UNMODIFIED reference's ``step()`` with an
external force per step and its floor (``resolve_collision``) -- against the NumPy model of tests/forces_cases.py within its
bound, which shows fixtures, model and bound sound without a device; the clamped-share condition from the stored shares; every
argument refusal of ``forces=`` and ``floor=``, which fire before the engine is touched; the engine calls with and without the
keywords on the recording double of tests/test_rollout_cpu.py; the new names of the C ABI."""
import inspect
import types

import numpy as np
import pytest

import forces_cases as fc
from conftest import load_golden
from pdsolve_cases import AMP_CAP, KS, MODES, host_case
from rollout_cases import START_FRAMES, start_state
from test_gpu_gstep import _case as gstep_case
from test_rollout_cpu import _rollout_calls

from animsnapbases_amd import _lib, dynamics
from animsnapbases_amd.posSnapshots import posSnapshots


def _fixture(name):
    z = load_golden("forces_" + name)
    floor = (float(z["floor"]), 1) if "floor" in z else None
    return z, floor


@pytest.mark.parametrize("name", sorted(fc.FIXTURES))
def test_host_model_matches_the_reference_steps(name):
    z, floor = _fixture(name)
    assert z["Ks"].tolist() == list(KS) and float(z["dt"]) == 0.5 and z["start_frames"].tolist() == START_FRAMES
    assert tuple(z["gravity"]) == fc.G and (floor is not None) == fc.FIXTURES[name]
    steps = z["steps"].tolist()
    assert steps and steps[0] == 1 and set(steps) <= set(fc.steps_of(name))
    _, frames, _, one = gstep_case(name)
    c = host_case(name)
    dt = float(z["dt"])
    acc = dt * dt * np.array(fc.G)
    force = z["force"]
    assert force.shape == (fc.T_S, frames.shape[1], 3) and np.array_equal(force, fc.force_of(frames.shape[1]))
    fa = fc.fa_of(force, c["masses"], dt)
    if floor is not None:
        assert floor[0] == fc.floor_of(name, frames, acc)
    for mode in MODES:
        s, x = start_state(frames, START_FRAMES, mode, acc)
        for K in KS:
            shares = []
            got = fc.rollout(c, K, max(steps), s, x, START_FRAMES, acc, fa, floor, shares=shares)
            bare = fc.rollout(c, K, max(steps), s, x, START_FRAMES, acc)
            stored = z["share_%s_%d" % (mode, K)]
            assert stored.shape == (max(steps),)
            if floor is None:
                assert not stored.any() and not any(shares)
            else:
                fc.check_shares(stored)                             # the reference's own count, at every step up to the last kept
                assert np.abs(stored - shares).max() <= 1.0 / stored.size / 10      # the model clamps the pairs the reference clamps
            for T in steps:
                amp = float(z["amp_%s_%d_%d" % (mode, K, T)])
                assert 0.0 < amp <= AMP_CAP
                ref = z["q_%s_%d_%d" % (mode, K, T)]
                assert ref.shape == x.shape and np.isfinite(ref).all()
                B = fc.bound_T(one[mode], K, T, amp, ref, acc, fa)
                err = np.abs(got[T - 1] - ref).max()                # over every start frame: none is left out
                print("%s %s K = %d T = %d: amp %.3g, share %.3f, max abs err %.3g, B %.3g, err / bound %.3g"
                      % (name, mode, K, T, amp, stored[T - 1], err, B, err / B))
                assert err <= B
                assert np.abs(bare[T - 1] - ref).max() > B          # without the force and the floor the model is somewhere else


def test_the_model_is_the_engines_arithmetic():
    rng = np.random.default_rng(0)
    s = rng.standard_normal((3, 5, 3))
    fa = rng.standard_normal((7, 5, 3))
    x, hit = fc.external(s, fc.rows_of(fa, [0, 3, 6]), (0.1, 2))
    want = s + fa[[0, 3, 6]]
    assert np.array_equal(hit, want[..., 2] < 0.1) and hit.any() and not hit.all()
    assert np.array_equal(x[..., :2], want[..., :2]) and np.array_equal(x[..., 2], np.maximum(want[..., 2], 0.1))
    assert np.array_equal(fc.external(s, None)[0], s) and np.array_equal(fc.external(s, fa[2])[0], s + fa[2][None])
    s[1, 2, 2] = np.nan                                             # a comparison, not a maximum: NaN stays
    assert np.isnan(fc.external(s, None, (0.1, 2))[0][1, 2, 2])
    m = 0.5 + rng.random(5)
    assert np.array_equal(fc.fa_of(fa, m, 0.25), 0.0625 * (fa / m[:, None]))


# ------------------------------------------------------------------ the keywords and their refusals
def test_the_positional_order_of_the_keywords():
    """``forces`` and ``floor`` stand directly in front of ``pins``, which tests/test_pins_cpu.py holds to the last place (in
    ``solve_frames`` to the place before ``hyper``); they are passed by name."""
    names = lambda m: list(inspect.signature(getattr(posSnapshots, m)).parameters)
    assert names("simulate_frames")[-3:] == ["forces", "floor", "pins"]
    assert names("reduced_rollout_errors")[-3:] == ["forces", "floor", "pins"]
    assert names("solve_frames")[-4:] == ["forces", "floor", "pins", "hyper"]
    for m in ("global_step", "global_solve_setup", "reduced_solve_errors", "reduced_global_step_errors", "subspace_solve_errors"):
        assert "forces" not in names(m) and "floor" not in names(m)
    for m in ("simulate_frames", "reduced_rollout_errors", "solve_frames"):
        p = inspect.signature(getattr(posSnapshots, m)).parameters
        assert p["forces"].default is None and p["floor"].default is None


def _bare(frs=6, N=5, multi=False):
    snaps = posSnapshots.__new__(posSnapshots)
    snaps._comm = types.SimpleNamespace(multi=multi)                # no engine: touching it is an AttributeError
    snaps.mass, snaps.global_matrix, snaps.test_verts, snaps.tris = None, None, None, None
    snaps.nVerts, snaps.frs = N, frs
    snaps.verts = np.random.default_rng(0).standard_normal((frs, N, 3))
    return snaps


def _callers(snaps, m):
    edge = dict(kind="edge_spring", elements=np.array([[0, 1], [1, 2]]))
    return {
        "simulate_frames": lambda T=2, **kw: snaps.simulate_frames([edge], 0.5, T, masses=m, **kw),
        "reduced_rollout_errors": lambda T=2, **kw: snaps.reduced_rollout_errors("edge_spring", {}, [1], 0.5, T, masses=m, elements=edge["elements"], **kw),
        "solve_frames": lambda T=1, **kw: snaps.solve_frames([edge], 0.5, masses=m, **kw),
    }


def test_arguments_checked_before_the_device_is_touched():
    N, frs = 5, 6
    snaps = _bare(frs, N)
    m = np.linspace(1.0, 2.0, N)
    ok = np.zeros((N, 3))
    for name, call in _callers(snaps, m).items():
        steps = 1 if name == "solve_frames" else 2
        bad_forces = [
            ("force", ok), ("force", [ok]), ("force", dict()), ("force", dict(vertices=[0])),
            ("unknown key", dict(force=ok, strength=2.0)),
            ("force of shape", dict(force=np.zeros((N, 2)))), ("force of shape", dict(force=np.zeros((N + 1, 3)))),
            ("force of shape", dict(force=np.zeros(3))), ("force of shape", dict(force=np.zeros((2, 2, N, 3)))),
            ("force of shape", dict(force=np.zeros((0, N, 3)))), ("force of shape", dict(force=np.full((N, 3), np.nan))),
            ("force of shape", dict(force=np.full((9, N, 3), np.inf))), ("force of shape", dict(force="push")),
            ("force of shape", dict(force=np.zeros((N, 3)), vertices=[0, 1])), ("force of shape", dict(force=np.zeros((9, 2, 3)), vertices=[0, 1, 2])),
            ("vertices", dict(force=np.zeros((1, 3)), vertices=[])), ("vertices", dict(force=np.zeros((1, 3)), vertices=[0.5])),
            ("vertices", dict(force=np.zeros((1, 3)), vertices=[[0]])),
            ("outside", dict(force=np.zeros((2, 3)), vertices=[0, N])), ("outside", dict(force=np.zeros((2, 3)), vertices=[-1, 0])),
            ("twice", dict(force=np.zeros((2, 3)), vertices=[3, 3])),
            ("start", dict(force=ok, start=-1)), ("start", dict(force=ok, start=1.0)), ("start", dict(force=ok, start=True)),
        ]
        for match, f in bad_forces:
            with pytest.raises(ValueError, match=match):
                call(forces=f)
        # the rows: the last selected frame is frs - 1; step t reads row start + f + t - 1
        need = frs - 1 + steps - 1
        with pytest.raises(ValueError, match="row %d of force is needed" % need):
            call(forces=dict(force=np.zeros((need, N, 3))))
        with pytest.raises(ValueError, match="row %d of force is needed" % (need + 3)):
            call(forces=dict(force=np.zeros((need + 3, N, 3)), start=3))
        with pytest.raises(ValueError, match="row %d of force is needed" % (2 + steps - 1)):
            call(forces=dict(force=np.zeros((2, 2, 3)), vertices=[0, 4]), frame_end=3)
        bad_floor = [("floor must be", 0.0), ("floor must be", dict()), ("floor must be", dict(axis=1)), ("unknown key", dict(height=0.0, y=1)),
                     ("height", dict(height=np.nan)), ("height", dict(height=np.inf)), ("height", dict(height="low")), ("height", dict(height=None)),
                     ("axis", dict(height=0.0, axis=3)), ("axis", dict(height=0.0, axis=-1)), ("axis", dict(height=0.0, axis=1.0)),
                     ("axis", dict(height=0.0, axis=True)), ("axis", dict(height=0.0, axis="y"))]
        for match, f in bad_floor:
            with pytest.raises(ValueError, match=match):
                call(floor=f)
        # masses that cannot divide a force
        with pytest.raises(ValueError, match="masses"):
            _callers(snaps, np.ones(N + 1))[name](forces=dict(force=ok))
        # a good pair passes every check and reaches the engine, which this object does not have (the sweep: its basis, read next)
        with pytest.raises(ValueError, match="basis dict") if name == "reduced_rollout_errors" else pytest.raises(AttributeError):
            call(forces=dict(force=np.zeros((need + 1, 2, 3)), vertices=[4, 0]), floor=dict(height=-1.0, axis=2))
    # the cap on the dense table, named with its size
    big = _bare(2, 2 ** 20)
    call = _callers(big, np.ones(2 ** 20))["simulate_frames"]
    with pytest.raises(ValueError, match="%d bytes" % (100 * 3 * 2 ** 20 * 8)):
        call(forces=dict(force=np.broadcast_to(np.zeros((1, 1, 3)), (100, 1, 3)), vertices=[5]))
    # several ranks
    many = _bare(multi=True)
    for name, call in _callers(many, m).items():
        with pytest.raises(NotImplementedError):
            call(forces=dict(force=ok), floor=dict(height=0.0))


def test_the_checked_records():
    N, frs = 5, 6
    snaps = _bare(frs, N)
    m = np.linspace(1.0, 2.0, N)
    ex = snaps._explicit("test", 0.25, "zero", (0.0, 0.0, 0.0), m)
    frames = snaps._frames("train", 0, None, 1)
    assert snaps._external("test", None, None, ex, frames) is None
    rng = np.random.default_rng(1)
    f = rng.standard_normal((9, N, 3))
    e = snaps._external("test", dict(force=f, start=2), dict(height=0.5), ex, frames, 2)
    assert isinstance(e, dynamics.External) and isinstance(e.forces, dynamics.Forces) and isinstance(e.floor, dynamics.Floor)
    assert e.floor == (0.5, 1) and e.forces.start == 2 and e.forces.table.shape == (9, 3 * N) and e.forces.table.flags["C_CONTIGUOUS"]
    assert np.array_equal(e.forces.table, fc.fa_of(f, m, 0.25).reshape(9, -1))      # the reference's order, f64
    c = snaps._external("test", dict(force=f[0]), None, ex, frames, 2)
    assert c.floor is None and c.forces.table.shape == (3 * N,) and np.array_equal(c.forces.table, e.forces.table[0])
    v = np.array([4, 1])
    sp = snaps._external("test", dict(force=f[:, :2], vertices=v), None, ex, frames, 2)
    dense = np.zeros_like(f)
    dense[:, v] = f[:, :2]
    assert np.array_equal(sp.forces.table, fc.fa_of(dense, m, 0.25).reshape(9, -1))
    only = snaps._external("test", None, dict(height=-2, axis=0), ex, frames)
    assert only.forces is None and only.floor == (-2.0, 0)


# ------------------------------------------------------------------ the engine calls
def test_engine_calls_with_and_without_the_keywords(monkeypatch):
    from test_dynamics_trace_cpu import _inputs, _kinds
    c, g = _inputs()[:2]
    tet, edge = _kinds()
    N, F = g["frames"].shape[1], g["frames"].shape[0]
    red = dict(tet, basis=c.basis, num_components=4, reduction=c.reduction)
    names = lambda calls: [n for n, _ in calls]
    force = np.random.default_rng(2).standard_normal((F + 8, N, 3))
    forces, floor = dict(force=force, start=3), dict(height=-0.2, axis=2)
    pins = dict(vertices=[0, 3], wi=2.0)
    sim = lambda **kw: (lambda s: s.simulate_frames([red, edge], 0.5, 3, num_iterations=2, frame_start=1, frame_jump=2, **kw))
    plain, _ = _rollout_calls(monkeypatch, sim())
    head = ["gstep_held", "gstep_setup", "rforce_operator"]
    slots = ["cproj_setup", "rforce_solver", "pdsolve_slot", "cproj_setup", "pdsolve_slot"]
    tail = 2 * ["pdsolve_iterate", "pdsolve_advance"] + ["pdsolve_iterate", "pdsolve_positions"]
    assert names(plain) == head + ["pdsolve_begin", "pdsolve_carry"] + slots + tail            # the sequence recorded today
    both, _ = _rollout_calls(monkeypatch, sim(forces=forces, floor=floor))
    assert names(both) == head + ["ext_set", "pdsolve_begin", "pdsolve_carry", "pdsolve_external"] + slots + tail
    table, fl = dict(both)["ext_set"]
    assert table.shape == (F + 8, 3 * N) and fl == (-0.2, 2) and dict(both)["pdsolve_external"] == (3,)
    # with pins: external stands before them
    pinned, _ = _rollout_calls(monkeypatch, sim(forces=forces, pins=pins))
    assert names(pinned) == head + ["pins_set", "ext_set", "pdsolve_begin", "pdsolve_carry", "pdsolve_external", "pdsolve_pins"] + slots + tail
    assert dict(pinned)["ext_set"][1] is None
    # floor only: no table, row 0
    low, _ = _rollout_calls(monkeypatch, sim(floor=floor))
    assert dict(low)["ext_set"] == (None, (-0.2, 2)) and dict(low)["pdsolve_external"] == (0,)
    # a continuation: external behind the advance that makes s_1
    import torch
    state = (torch.zeros((len(range(1, F, 2)), N, 3), dtype=torch.float64),) * 2
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: types.SimpleNamespace(synchronize=lambda: None))
    monkeypatch.setattr(posSnapshots, "_rollout_state", lambda *a: None)
    cont, _ = _rollout_calls(monkeypatch, sim(forces=forces, pins=pins, state=state))
    assert names(cont) == head + ["pins_set", "ext_set", "pdsolve_begin", "pdsolve_carry", "pdsolve_advance", "pdsolve_external",
                                  "pdsolve_pins"] + slots + tail
    # solve_frames: row start + f, bound behind the begin
    solve = lambda **kw: (lambda s: s.solve_frames([edge], 0.5, num_iterations=2, **kw))
    plain, _ = _rollout_calls(monkeypatch, solve())
    assert names(plain) == ["gstep_held", "gstep_setup", "pdsolve_begin", "cproj_setup", "pdsolve_slot", "pdsolve_iterate"]
    got, _ = _rollout_calls(monkeypatch, solve(forces=dict(force=force[0]), pins=pins))
    assert names(got) == ["gstep_held", "gstep_setup", "pins_set", "ext_set", "pdsolve_begin", "pdsolve_external", "pdsolve_pins", "cproj_setup",
                          "pdsolve_slot", "pdsolve_iterate"]
    assert dict(got)["ext_set"][0].shape == (3 * N,)
    # the sweep binds them in the full roll-out and in every reduced one
    from test_dynamics_trace_cpu import _reduced_kw
    sweep, _ = _rollout_calls(monkeypatch, lambda s: s.reduced_rollout_errors("tets_strain", c.basis, [2, 4], 0.5, 2, num_iterations=2, forces=forces,
                                                                              floor=floor, **_reduced_kw()))
    assert names(sweep).count("ext_set") == 1 and names(sweep).count("pdsolve_external") == 3         # one upload, a binding per roll-out
    bare, _ = _rollout_calls(monkeypatch, lambda s: s.reduced_rollout_errors("tets_strain", c.basis, [2, 4], 0.5, 2, num_iterations=2, **_reduced_kw()))
    assert names(bare) == [n for n in names(sweep) if n not in ("ext_set", "pdsolve_external")]
    assert names(sweep).index("ext_set") < names(sweep).index("pdsolve_begin")


def test_simulate_subspace_takes_forces_and_refuses_a_floor(monkeypatch):
    names = list(inspect.signature(posSnapshots.simulate_subspace).parameters)
    assert names[-3:] == ["pins", "forces", "floor"]                # no existing test holds this method's last place: the issue's order
    snaps = _bare()
    snaps._global_solver, snaps._global_subspace = ("subspace", None), (np.eye(5)[:, :2].reshape(5, 2, 1).repeat(3, axis=2), None)
    edge = dict(kind="edge_spring", elements=np.array([[0, 1]]), basis={}, num_components=1)
    with pytest.raises(ValueError) as e:
        snaps.simulate_subspace([edge], 0.5, 2, masses=np.ones(5), floor=dict(height=0.0))
    msg = str(e.value)
    assert "no form in the subspace coordinates z" in msg and "O(N) pass" in msg and "simulate_frames" in msg and "set_global_solver('subspace')" in msg
    for bad, match in ((dict(force=np.zeros((4, 3))), "force of shape"), (dict(force=np.zeros((5, 3)), start=-1), "start"),
                       (dict(force=np.zeros((6, 5, 3))), "row 6 of force is needed")):
        with pytest.raises(ValueError, match=match):
            snaps.simulate_subspace([edge], 0.5, 2, masses=np.ones(5), forces=bad)
    many = _bare(multi=True)
    with pytest.raises(NotImplementedError):
        many.simulate_subspace([edge], 0.5, 2, masses=np.ones(5), forces=dict(force=np.zeros((5, 3))))


def test_new_abi_names_are_declared():
    for name in ("asb_ext_set", "asb_ext_clear", "asb_pdsolve_external", "asb_zroll_forces"):
        assert name in _lib.PROTOTYPES
        assert hasattr(_lib.load(), name)
