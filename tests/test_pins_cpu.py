"""CPU: positional constraints (pins).  The fixtures of tools/gen_golden_pins.py -- the UNMODIFIED reference's ``step()`` written
out with its ``PositionalConstraint`` objects and the step counter it hands ``get_pi`` -- against the NumPy model of
tests/pins_cases.py within the bound of that module, which shows fixtures and bounds sound without a device; ``global_matrix``
and ``pins_ST`` against the reference's matrix; every refusal of the ``pins=`` dict, before the engine is touched; the engine
calls with and without pins on a recording double; the new names of the C ABI."""
import inspect
import types

import numpy as np
import pytest

import pins_cases as pins
from conftest import load_golden
from pdsolve_cases import AMP_CAP, KS, MODES, parts_of
from rollout_cases import START_FRAMES, adv_bound, bound_T, start_state
from test_gpu_cforces import _bound as force_bound, _g
from test_gpu_cproj import RAW_TOL

from animsnapbases_amd import _lib, projections as proj
from animsnapbases_amd.posSnapshots import posSnapshots

METHODS = ["constraint_forces", "global_solve_setup", "global_step", "reduced_global_step_errors", "solve_frames", "reduced_solve_errors",
           "simulate_frames", "reduced_rollout_errors"]


def kinds_force_bound(name, tol_p=RAW_TOL):
    """The force bound of the element set of a fixture at its frames' projections (tests/test_gpu_cforces.py)."""
    if pins.FIXTURES[name]["base"] == "combined":
        c = load_golden("st_combined")
        return force_bound(_g("edge_spring")[2], c["p_edge"], tol_p) + force_bound(_g("tets_strain")[2], _g("tets_strain")[0]["expected"], tol_p)
    g, _, St = _g(pins.FIXTURES[name]["base"])
    return force_bound(St, g["expected"], tol_p)


# ------------------------------------------------------------------ 1. the host model against the reference
@pytest.mark.parametrize("name", sorted(pins.FIXTURES))
def test_host_model_matches_the_reference(name):
    z = load_golden("pins_" + name)
    fx = pins.FIXTURES[name]
    assert z["Ks"].tolist() == list(KS) and float(z["dt"]) == 0.5 and float(z["wi"]) == pins.WI
    assert z["start_frames"].tolist() == START_FRAMES and z["gravity"].tolist() == list(pins.G)
    assert z["vertices"].tolist() == list(fx["vertices"]) and z["pin_wi"].tolist() == list(fx["wi"])
    assert ("shift" in z) == fx["moving"] and (not fx["moving"] or z["shift"].shape == (pins.T_S, len(fx["vertices"]), 3))
    steps = z["steps"].tolist()
    assert steps and steps[0] == 1 and set(steps) <= set(pins.steps_of(name))
    c = pins.host_case(name)
    free = pins.with_pins(c, dict(vertices=c["pins"][0], wi=0.0, positions=c["pins"][2]))       # the same model, weightless pins
    frames = c["frames"]
    acc = c["dt"] ** 2 * np.array(pins.G)
    fb = kinds_force_bound(name)
    for mode in MODES:
        s, x = start_state(frames, START_FRAMES, mode, acc)
        ref = z["g_" + mode]
        one = pins.one_bound(c, fb, np.abs(ref).max(), START_FRAMES)
        err = np.abs(pins.iterate(c, s, x, 1, START_FRAMES) - ref).max()
        print("%s %s global step: max abs err %.3g, bound %.3g" % (name, mode, err, 2 * one))
        assert err <= 2 * one
        assert np.abs(pins.iterate(free, s, x, 1, START_FRAMES) - ref).max() > 2 * one          # the pins matter
        for K in KS:
            got = pins.rollout(c, K, max(steps), s, x, START_FRAMES, acc)
            loose = pins.rollout(free, K, max(steps), s, x, START_FRAMES, acc)
            for T in steps:
                amp = float(z["amp_%s_%d_%d" % (mode, K, T)])
                assert 0.0 < amp <= AMP_CAP
                ref = z["q_%s_%d_%d" % (mode, K, T)]
                assert ref.shape == x.shape and np.isfinite(ref).all()
                one = pins.one_bound(c, fb, np.abs(ref).max(), START_FRAMES)
                B = bound_T(one, K, T, amp, adv_bound(ref, ref, acc))
                err = np.abs(got[T - 1] - ref).max()                # over every start frame: none is left out
                print("%s %s K = %d T = %d: amp %.3g, max abs err %.3g, B %.3g, err / bound %.3g" % (name, mode, K, T, amp, err, B, err / B))
                assert err <= B
                assert np.abs(loose[T - 1] - ref).max() > B         # without the pins the model is somewhere else


def test_the_moving_fixture_reads_the_row_of_the_step_counter():
    """Row f for the step from frame f, one more per step: another convention misses the fixture by far more than the bound."""
    name = "combined_moving"
    z, c = load_golden("pins_" + name), pins.host_case(name)
    acc = c["dt"] ** 2 * np.array(pins.G)
    s, x = start_state(c["frames"], START_FRAMES, "difference", acc)
    T = max(z["steps"].tolist())
    ref = z["q_difference_3_%d" % T]
    B = bound_T(pins.one_bound(c, kinds_force_bound(name), np.abs(ref).max(), START_FRAMES), 3, T, float(z["amp_difference_3_%d" % T]),
                adv_bound(ref, ref, acc))
    rows = np.array(START_FRAMES)
    assert np.abs(pins.rollout(c, 3, T, s, x, rows, acc)[T - 1] - ref).max() <= B
    for wrong in (rows + 1, np.zeros_like(rows)):
        assert np.abs(pins.rollout(c, 3, T, s, x, wrong, acc)[T - 1] - ref).max() > B


# ------------------------------------------------------------------ 2. the host's matrix and S^T
@pytest.mark.parametrize("name", sorted(pins.FIXTURES))
def test_global_matrix_with_pins_is_the_references(name):
    from scipy import sparse
    z, c = load_golden("pins_" + name), pins.host_case(name)
    N = c["masses"].shape[0]
    ref = sparse.coo_matrix((z["val"], (z["row"], z["col"])), shape=tuple(z["shape"])).toarray()
    A = c["A"]
    assert A.has_sorted_indices and abs(A - A.T).max() == 0.0
    assert np.abs(A.toarray() - ref).max() <= 8 * pins.EPS * np.abs(ref).max()
    v, w = c["pins"][:2]
    plain = proj.global_matrix([(k[0], pins.WI) for k in c["kinds"]], N, c["masses"], c["dt"])
    d = (A - plain).toarray()
    assert np.count_nonzero(d - np.diag(np.diag(d))) == 0 and np.allclose(np.diag(d)[v], w, rtol=1e-13) and np.count_nonzero(np.diag(d)) == v.size
    # the pattern is the one without pins: the slab plan is not affected
    assert np.array_equal(A.indptr, plain.indptr) and np.array_equal(A.indices, plain.indices)
    # callers without pins get what they got
    again = proj.global_matrix([(k[0], pins.WI) for k in c["kinds"]], N, c["masses"], c["dt"], None)
    assert np.array_equal(again.data, plain.data) and np.array_equal(again.indices, plain.indices)
    St = proj.pins_ST(v, w, N)
    assert St.shape == (N, v.size) and St.nnz == v.size and St.has_sorted_indices
    assert np.array_equal(St.toarray()[v, np.arange(v.size)], w)
    assert np.array_equal(St @ pins.targets(c, [5])[0], pins.pin_term(c, [5])[0])
    for bad in (([0, 0], 1.0), ([0, N], 1.0), ([-1], 1.0), ([], 1.0), ([1], -1.0), ([1], np.nan)):
        with pytest.raises(ValueError, match="pins"):
            proj.pins_ST(bad[0], bad[1], N)
        with pytest.raises(ValueError, match="pins"):
            proj.global_matrix([(k[0], pins.WI) for k in c["kinds"]], N, c["masses"], c["dt"], bad)


# ------------------------------------------------------------------ 3. the keyword and its refusals
def test_pins_is_the_last_keyword_of_the_eight_methods():
    """... of six of them.  ``solve_frames`` and ``reduced_solve_errors`` keep ``hyper`` last, which tests/test_hyper_cpu.py holds
    them to: there ``pins`` stands directly before it, behind every keyword the methods had before ``hyper``."""
    for m in METHODS:
        params = list(inspect.signature(getattr(posSnapshots, m)).parameters.values())
        names = [p.name for p in params]
        if m in ("solve_frames", "reduced_solve_errors"):
            assert names[-2:] == ["pins", "hyper"], m
        else:
            assert names[-1] == "pins", m
        assert params[names.index("pins")].default is None, m


def _bare(frs=6, N=5):
    snaps = posSnapshots.__new__(posSnapshots)
    snaps._comm = types.SimpleNamespace(multi=False)              # no engine: touching it is an AttributeError
    snaps.mass, snaps.global_matrix, snaps.test_verts, snaps.tris = None, None, None, None
    snaps.nVerts, snaps.frs = N, frs
    snaps.verts = np.random.default_rng(0).standard_normal((frs, N, 3))
    return snaps


def _callers(snaps):
    m = np.ones(snaps.nVerts)
    edge = dict(kind="edge_spring", elements=np.array([[0, 1], [1, 2]]))
    red = dict(elements=edge["elements"])
    return {
        "constraint_forces": lambda p, **kw: snaps.constraint_forces([edge], pins=p, **kw),
        "global_solve_setup": lambda p, **kw: snaps.global_solve_setup([edge], 0.5, m, pins=p),
        "global_step": lambda p, **kw: snaps.global_step([edge], 0.5, m, pins=p, **kw),
        "reduced_global_step_errors": lambda p, **kw: snaps.reduced_global_step_errors("edge_spring", {}, [1], 0.5, m, pins=p, **red, **kw),
        "solve_frames": lambda p, **kw: snaps.solve_frames([edge], 0.5, 2, m, pins=p, **kw),
        "reduced_solve_errors": lambda p, **kw: snaps.reduced_solve_errors("edge_spring", {}, [1], 0.5, 2, m, pins=p, **red, **kw),
        "simulate_frames": lambda p, **kw: snaps.simulate_frames([edge], 0.5, kw.pop("num_steps", 2), 2, m, pins=p, **kw),
        "reduced_rollout_errors": lambda p, **kw: snaps.reduced_rollout_errors("edge_spring", {}, [1], 0.5, kw.pop("num_steps", 2), 2, m, pins=p,
                                                                                **red, **kw),
    }


@pytest.mark.parametrize("method", METHODS)
def test_every_refusal_fires_before_the_device_is_touched(method):
    snaps = _bare()
    N = snaps.nVerts
    call = _callers(snaps)[method]
    good = dict(vertices=[0, 3], wi=1.0)
    bad = [
        ("pins must be a dict", [0, 3]),
        ("pins must be a dict", dict(wi=1.0)),
        ("pins must be a dict", dict(vertices=[0])),
        ("unknown key", dict(good, weight=2.0)),
        ("vertices", dict(good, vertices=[])),
        ("vertices", dict(good, vertices=[[0, 3]])),
        ("vertices", dict(good, vertices=[0.0, 3.0])),
        ("outside", dict(good, vertices=[0, N])),
        ("outside", dict(good, vertices=[-1, 2])),
        ("twice", dict(good, vertices=[3, 0, 3])),
        ("wi", dict(good, wi=[1.0, 2.0, 3.0])),
        ("wi", dict(good, wi=[[1.0, 2.0]])),
        ("wi", dict(good, wi=-1.0)),
        ("wi", dict(good, wi=[1.0, np.inf])),
        ("wi", dict(good, wi=np.nan)),
        ("wi", dict(good, wi="stiff")),
        ("positions", dict(good, positions=np.zeros((3, 3)))),
        ("positions", dict(good, positions=np.zeros((2, 2)))),
        ("positions", dict(good, positions=[[0.0, 0.0, np.nan], [0.0, 0.0, 0.0]])),
        ("shift", dict(good, shift=np.zeros((9, 3, 3)))),
        ("shift", dict(good, shift=np.zeros((9, 2)))),
        ("shift", dict(good, shift=np.zeros(9))),
        ("shift", dict(good, shift=np.zeros((0, 3)))),
        ("shift", dict(good, shift=np.full((9, 2, 3), np.inf))),
        ("shift_start", dict(good, shift_start=-1)),
        ("shift_start", dict(good, shift_start=1.0)),
        ("shift_start", dict(good, shift_start=True)),
    ]
    for match, p in bad:
        with pytest.raises(ValueError, match=match):
            call(p)
    if method == "global_solve_setup":
        return
    # the rows a call needs: frame f reads row shift_start + f, step t of a roll-out one more each
    steps = 3 if method in ("simulate_frames", "reduced_rollout_errors") else 1
    kw = dict(num_steps=steps) if steps > 1 else {}
    last = snaps.frs - 1 + steps - 1
    for shape in ((last, 3), (last, 2, 3)):                           # one row short
        with pytest.raises(ValueError, match="row %d of shift" % last):
            call(dict(good, shift=np.zeros(shape)), **dict(kw))
    with pytest.raises(ValueError, match="row %d of shift" % (last + 4)):
        call(dict(good, shift=np.zeros((last + 4, 3)), shift_start=4), **dict(kw))
    with pytest.raises(ValueError, match="row %d of shift" % (2 + steps - 1)):        # the LAST selected frame counts: range(0, 4, 2)
        call(dict(good, shift=np.zeros((2 + steps - 1, 3))), frame_end=4, frame_jump=2, **dict(kw))
    # enough rows: the call gets past the pins -- as far as the engine, which the bare object does not have, or, in a sweep, as
    # far as its empty basis
    passed = lambda: pytest.raises(ValueError, match="basis dict") if method.startswith("reduced_") else pytest.raises(AttributeError)
    with passed():
        call(dict(good, shift=np.zeros((last + 1, 3))), **dict(kw))
    with passed():
        call(dict(good, shift=np.zeros((3 + steps - 1, 2, 3))), frame_end=4, frame_jump=2, **dict(kw))


def test_the_record_of_a_call():
    snaps = _bare()
    p = snaps._pins("t", dict(vertices=(4, 1), wi=2.0))
    assert p.vertices.tolist() == [4, 1] and p.vertices.dtype == np.int64 and p.wi.tolist() == [2.0, 2.0] and p.shift is None and p.start == 0
    assert np.array_equal(p.p0, snaps.verts[0][[4, 1]])              # the rest positions _setup would take
    assert np.array_equal(p.St.toarray(), proj.pins_ST([4, 1], 2.0, 5).toarray())
    sh = np.arange(42.0).reshape(7, 2, 3)
    p = snaps._pins("t", dict(vertices=np.array([4, 1]), wi=[0.0, 3.0], positions=np.ones((2, 3)), shift=sh, shift_start=np.int64(2)))
    assert p.wi.tolist() == [0.0, 3.0] and np.array_equal(p.shift, sh) and p.start == 2 and np.array_equal(p.p0, np.ones((2, 3)))
    assert snaps._pins("t", None) is None
    snaps.verts, snaps._snapTensor = None, None                      # an adopted tensor: frame 0 back in world space
    snaps.snapTensor = np.full((6, 5, 3), 6.0)
    snaps.pre_scale_factor, snaps._standarize, snaps.mean = 2.0, True, np.ones((5, 3))
    assert np.array_equal(snaps._pins("t", dict(vertices=[2], wi=1.0)).p0, np.full((1, 3), 4.0))


# ------------------------------------------------------------------ 4. the engine calls
def _calls(monkeypatch, fn):
    from test_rollout_cpu import _rollout_calls
    calls, out = _rollout_calls(monkeypatch, fn)
    return [n for n, _ in calls], calls, out


def _trace_inputs():
    from test_dynamics_trace_cpu import _inputs, _kinds, _reduced_kw
    c = _inputs()[0]
    tet, edge = _kinds()
    return c, tet, edge, dict(tet, basis=c.basis, num_components=4, reduction=c.reduction), _reduced_kw


def test_without_pins_the_engine_calls_are_todays(monkeypatch):
    """``pins=None`` spelled out gives the sequence of the call without the keyword, argument for argument, and no pin call."""
    from test_dynamics_trace_cpu import _digest
    c, tet, edge, red, rkw = _trace_inputs()
    cases = [
        lambda s, **kw: s.constraint_forces([tet, edge], frame_start=1, frame_jump=2, **kw),
        lambda s, **kw: s.solve_frames([red, edge], 0.5, num_iterations=3, start="frame", frame_jump=2, **kw),
        lambda s, **kw: s.solve_frames([red], 0.5, num_iterations=3, hyper="touched", **kw),
        lambda s, **kw: s.reduced_solve_errors("tets_strain", c.basis, [2, 4], 0.5, num_iterations=2, **rkw(), **kw),
        lambda s, **kw: s.simulate_frames([red, edge], 0.5, 3, num_iterations=2, record_every=1, **kw),
        lambda s, **kw: s.reduced_rollout_errors("tets_strain", c.basis, [2], 0.5, 3, num_iterations=2, hyper="touched", **rkw(), **kw),
    ]
    new = {"pins_set", "pins_clear", "pins_term", "fm_add", "pdsolve_pins"}
    pointer = lambda a: isinstance(a, int) and not isinstance(a, bool) and a > (1 << 20)
    for fn in cases:
        a, ca, _ = _calls(monkeypatch, fn)
        b, cb, _ = _calls(monkeypatch, lambda s: fn(s, pins=None))
        assert a == b and not new & set(a)
        for (_, x), (_, y) in zip(ca, cb):                           # (device pointers differ from run to run)
            assert [None if pointer(v) else _digest(v) for v in x] == [None if pointer(v) else _digest(v) for v in y]


def test_with_pins_the_new_calls_appear_where_specified(monkeypatch):
    c, tet, edge, red, rkw = _trace_inputs()
    sh = np.zeros((140, 2, 3))
    P = dict(vertices=[0, 5], wi=[0.7, 1e3], shift=sh, shift_start=3)
    # constraint_forces: the pins' term behind the kinds', accumulated
    names, calls, out = _calls(monkeypatch, lambda s: s.constraint_forces([tet, edge], frame_start=1, frame_jump=2, pins=P))
    assert names == 2 * ["cproj_setup", "cforce_run"] + ["pins_set", "pins_term"]
    args = dict(calls)
    assert args["pins_term"][:5] == (1, 130, 2, 3, True) and args["pins_term"][5] == out[0].data_ptr()
    v, w, p0, shift = args["pins_set"]
    assert v.tolist() == [0, 5] and w.tolist() == [0.7, 1e3] and p0.shape == (2, 3) and shift is not None and shift.shape == sh.shape
    # a solve: pins_set before begin, pdsolve_pins directly after it; the matrix holds the weights
    names, calls, _ = _calls(monkeypatch, lambda s: s.solve_frames([red, edge], 0.5, num_iterations=3, start="frame", frame_jump=2, pins=P))
    assert names == ["gstep_held", "gstep_setup", "rforce_operator", "pins_set", "pdsolve_begin", "pdsolve_pins", "cproj_setup", "rforce_solver",
                     "pdsolve_slot", "cproj_setup", "pdsolve_slot", "pdsolve_iterate"]
    assert dict(calls)["pdsolve_pins"] == (3,)
    A = dict(calls)["gstep_setup"][0]
    _, _, plain = _calls(monkeypatch, lambda s: (s.global_solve_setup([tet, edge], 0.5), s.global_matrix)[1])
    d = (A - plain).toarray()
    assert np.allclose(np.diag(d)[[0, 5]], [0.7, 1e3], rtol=1e-12) and np.count_nonzero(d) == 2
    # hyper: every KIND reduced; the pins ride along and take no slot
    names, calls, _ = _calls(monkeypatch, lambda s: s.solve_frames([red], 0.5, num_iterations=3, hyper="touched", pins=P))
    assert names == ["gstep_held", "gstep_setup", "rforce_operator", "hyper_operator", "pins_set", "pdsolve_begin", "pdsolve_pins", "cproj_setup",
                     "rforce_solver", "pdsolve_slot", "hyper_iterate"]
    # a roll-out: once per call, the advances carry the row on by themselves
    names, calls, _ = _calls(monkeypatch, lambda s: s.simulate_frames([edge], 0.5, 3, num_iterations=2, pins=P))
    assert names == ["gstep_held", "gstep_setup", "pins_set", "pdsolve_begin", "pdsolve_carry", "pdsolve_pins", "cproj_setup", "pdsolve_slot",
                     "pdsolve_iterate", "pdsolve_advance", "pdsolve_iterate", "pdsolve_advance", "pdsolve_iterate", "pdsolve_positions"]
    # the sweeps: every solve and roll-out of the sweep binds the pins
    names, _, _ = _calls(monkeypatch, lambda s: s.reduced_solve_errors("tets_strain", c.basis, [2, 4], 0.5, num_iterations=2, pins=P, **rkw()))
    run = lambda solver: ["pins_set", "pdsolve_begin", "pdsolve_pins", "cproj_setup"] + solver + ["pdsolve_slot", "pdsolve_iterate"]
    assert names == ["gstep_held", "gstep_setup"] + run([]) + ["rforce_operator"] + 2 * (run(["rforce_solver"]) + ["force_diff"])
    names, _, _ = _calls(monkeypatch, lambda s: s.reduced_rollout_errors("tets_strain", c.basis, [2], 0.5, 2, num_iterations=2, pins=P, **rkw()))
    roll = lambda solver: ["pins_set", "pdsolve_begin", "pdsolve_carry", "pdsolve_pins", "cproj_setup"] + solver \
        + ["pdsolve_slot", "pdsolve_iterate", "pdsolve_advance", "pdsolve_iterate", "pdsolve_positions"]
    assert names == ["gstep_held", "gstep_setup"] + roll([]) + ["rforce_operator"] + roll(["rforce_solver"]) + 2 * ["force_diff"]


def test_pins_leave_their_selection_matrix(monkeypatch):
    _, tet, edge, _, _ = _trace_inputs()
    P = dict(vertices=[0, 5], wi=[0.7, 1e3])
    from test_rollout_cpu import Recorder
    from test_dynamics_trace_cpu import _bare as bare_snaps
    import torch
    real = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **kw: real(*a, **kw))
    snaps = bare_snaps(Recorder())
    snaps.constraint_forces([tet, edge], pins=P)
    assert list(snaps.assembly_ST) == ["tets_strain", "edge_spring", "positional"]
    assert np.array_equal(snaps.assembly_ST["positional"].toarray(), proj.pins_ST([0, 5], [0.7, 1e3], snaps.nVerts).toarray())
    snaps.constraint_forces([tet, edge])
    assert list(snaps.assembly_ST) == ["tets_strain", "edge_spring"]


def test_new_abi_names_are_declared():
    for name in ("asb_pins_set", "asb_pins_clear", "asb_pins_term", "asb_fm_add", "asb_pdsolve_pins"):
        assert name in _lib.PROTOTYPES
        assert hasattr(_lib.load(), name)
