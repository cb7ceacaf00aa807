"""CPU: the fixtures of tools/gen_golden_rollout.py -- the positions after T time steps of the UNMODIFIED reference's code
(``reference_loop`` per step, Simulators.py:531-532 between steps) from the start frames range(0, 130, 3) -- against the NumPy
model of tests/rollout_cases.py within B = 2 max(1, amp_T) T (K one + adv), which shows fixtures and bounds sound without a
device; the argument checks of ``posSnapshots.simulate_frames`` and ``reduced_rollout_errors``, which fire before the engine
is touched; the engine calls of a roll-out, in order, on a recording double; the new names of the C ABI."""
import types

import numpy as np
import pytest

from conftest import load_golden
from pdsolve_cases import host_case
from rollout_cases import AMP_CAP, KS, LONG, MODES, NAMES, REDUCED, START_FRAMES, STEPS, adv_bound, bound_T, rollout, start_state
from test_gpu_gstep import _case as gstep_case

from animsnapbases_amd import _lib
from animsnapbases_amd.posSnapshots import posSnapshots


@pytest.mark.parametrize("name", NAMES)
def test_host_model_matches_the_reference_rollout(name):
    z = load_golden("rollout_" + name)
    assert z["Ks"].tolist() == list(KS) and float(z["dt"]) == 0.5 and float(z["wi"]) == 0.7
    assert z["steps"].tolist() == list(STEPS[name]) and z["start_frames"].tolist() == START_FRAMES
    _, frames, _, one = gstep_case(name)
    c = host_case(name)
    one_step = load_golden("pdsolve_" + name)
    for mode in MODES:
        s, x = start_state(frames, START_FRAMES, mode)
        for K in KS:
            got = rollout(c, K, max(STEPS[name]), s, x)
            # T = 1 is the existing pdsolve fixture
            assert np.abs(got[0] - one_step["q_%s_%d" % (mode, K)][START_FRAMES]).max() <= bound_T(
                one[mode], K, 1, float(one_step["amp_%s_%d" % (mode, K)]), 0.0)
            for T in STEPS[name]:
                amp = float(z["amp_%s_%d_%d" % (mode, K, T)])
                assert 0.0 < amp <= AMP_CAP
                ref = z["q_%s_%d_%d" % (mode, K, T)]
                assert ref.shape == x.shape and np.isfinite(ref).all()
                B = bound_T(one[mode], K, T, amp, adv_bound(ref, ref))
                err = np.abs(got[T - 1] - ref).max()                # over every start frame: none is left out
                print("%s %s K = %d T = %d: amp %.3g, max abs err %.3g, B %.3g, err / bound %.3g" % (name, mode, K, T, amp, err, B, err / B))
                assert err <= B
                # the steps move: the fixture tells T steps from one
                assert np.abs(ref - one_step["q_%s_%d" % (mode, K)][START_FRAMES]).max() > B


@pytest.mark.parametrize("fixture", sorted(REDUCED))
def test_reduced_fixtures_hold_the_amplification_of_the_kept_steps(fixture):
    z = load_golden("rollout_reduced_" + fixture)
    steps = z["steps"].tolist()
    assert steps == list(LONG[:len(steps)])
    for m in z["ms"].tolist():
        for mode in MODES:
            for K in KS:
                for T in steps:
                    assert 0.0 < float(z["amp_%d_%s_%d_%d" % (m, mode, K, T)]) <= AMP_CAP


def _bare(multi):
    snaps = posSnapshots.__new__(posSnapshots)
    snaps._comm = types.SimpleNamespace(multi=multi)
    return snaps


def test_several_ranks_are_refused():
    g = load_golden("cproj_tets_strain")
    kinds = [dict(kind="tets_strain", elements=g["elements"])]
    snaps = _bare(True)
    with pytest.raises(NotImplementedError):
        snaps.simulate_frames(kinds, 0.5, 2, masses=np.ones(g["rest"].shape[0]))
    with pytest.raises(NotImplementedError):
        snaps.reduced_rollout_errors("tets_strain", {}, [1], 0.5, 2, masses=np.ones(g["rest"].shape[0]))


def test_arguments_checked_before_the_device_is_touched():
    import torch
    snaps = _bare(False)                                            # no engine: touching it is an AttributeError
    snaps.mass, snaps.global_matrix = None, None
    m = np.ones(4)
    edge = dict(kind="edge_spring", elements=np.array([[0, 1]]))
    for call in (lambda **kw: snaps.simulate_frames([edge], kw.pop("dt", 0.5), kw.pop("num_steps", 2), **kw),
                 lambda **kw: snaps.reduced_rollout_errors("edge_spring", {}, [1], kw.pop("dt", 0.5), kw.pop("num_steps", 2), **kw)):
        with pytest.raises(ValueError, match="masses"):
            call()
        with pytest.raises(ValueError, match="velocity"):
            call(masses=m, velocity="leapfrog")
        with pytest.raises(ValueError, match="gravity"):
            call(masses=m, gravity=(0.0, np.nan, 0.0))
        with pytest.raises(ValueError, match="dt"):
            call(masses=m, dt=0.0)
        for K in (0, -1, 2.5, None, "ten"):
            with pytest.raises(ValueError, match="num_iterations"):
                call(masses=m, num_iterations=K)
        for T in (0, -1, 2.5, None, "two", True):
            with pytest.raises(ValueError, match="num_steps"):
                call(masses=m, num_steps=T)
        for r in (0, -2, 1.5, "one"):
            with pytest.raises(ValueError, match="record_every"):
                call(masses=m, record_every=r)
        with pytest.raises(ValueError, match="hyper"):
            call(masses=m, hyper="some")
        with pytest.raises(TypeError):
            call(masses=m, history=True)                            # not offered
    with pytest.raises(ValueError, match="record_every"):
        snaps.reduced_rollout_errors("edge_spring", {}, [1], 0.5, 2, masses=m, record_every=None)
    with pytest.raises(ValueError, match="hyper"):                  # hyper needs the one kind reduced
        snaps.simulate_frames([edge], 0.5, 2, masses=m, hyper="touched")
    host = torch.zeros((1, 4, 3), dtype=torch.float64)
    for bad in (host, (host, host), (host,), [host, host, host], (np.zeros((1, 4, 3)),) * 2, "rest",
                (torch.zeros((1, 4, 3), dtype=torch.float32),) * 2):
        with pytest.raises(ValueError, match="state"):
            snaps.simulate_frames([edge], 0.5, 2, masses=m, state=bad)
    snaps.nVerts, snaps.frs, snaps.verts, snaps.tris = 4, 3, np.zeros((3, 4, 3)), None
    with pytest.raises(ValueError, match="unknown key"):
        snaps.simulate_frames([dict(edge, stiffness=2.0)], 0.5, 2, masses=m)
    with pytest.raises(ValueError, match="num_components"):
        snaps.simulate_frames([dict(edge, basis={})], 0.5, 2, masses=m)
    with pytest.raises(ValueError, match="second reduced kind"):
        snaps.simulate_frames([dict(edge, basis={}, num_components=1),
                               dict(kind="tris_strain", elements=np.array([[0, 1, 2]]), basis={}, num_components=1)], 0.5, 2, masses=m)
    with pytest.raises(ValueError, match="non-empty list"):
        snaps.simulate_frames([], 0.5, 2, masses=m)
    with pytest.raises(ValueError, match="empty frame range"):
        snaps.simulate_frames([edge], 0.5, 2, masses=m, frame_start=3)


# ------------------------------------------------------------------ the engine calls of a roll-out
class Recorder(object):
    """Records the name and the arguments of every engine method called."""
    device_id = 0

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*args, **kw):
            self.calls.append((name, args))
            if name == "gstep_setup":
                return 0.0
            if name == "force_diff":
                return np.ones(3), 1.0, np.ones(4), None
            return None
        return call


def _rollout_calls(monkeypatch, fn):
    import torch
    from test_dynamics_trace_cpu import _bare as bare_snaps
    real = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **kw: real(*a, **kw))
    eng = Recorder()
    out = fn(bare_snaps(eng))
    return eng.calls, out


def test_engine_calls_of_simulate_frames(monkeypatch):
    from test_dynamics_trace_cpu import _inputs, _kinds
    c = _inputs()[0]
    tet, edge = _kinds()
    red = dict(tet, basis=c.basis, num_components=4, reduction=c.reduction)
    names = lambda calls: [n for n, _ in calls]
    # two kinds, one of them reduced, the full path: five steps, a record every second one
    calls, out = _rollout_calls(monkeypatch, lambda s: s.simulate_frames([red, edge], 0.5, 5, num_iterations=3, gravity=(0.0, -9.81, 0.0),
                                                                         frame_start=1, frame_jump=2, record_every=2, chunk_frames=16))
    assert names(calls) == ["gstep_held", "gstep_setup", "rforce_operator", "pdsolve_begin", "pdsolve_carry", "cproj_setup", "rforce_solver",
                            "pdsolve_slot", "cproj_setup", "pdsolve_slot"] + 4 * ["pdsolve_iterate", "pdsolve_advance"] \
        + ["pdsolve_iterate", "pdsolve_positions"]
    q, q_prev, nF, (records, steps) = out
    assert steps == [2, 4] and tuple(records.shape) == (2, nF) + tuple(q.shape[1:]) and q.shape == q_prev.shape
    begin = dict(calls)["pdsolve_begin"]
    assert begin[10:] == (0, None) and begin[8] == 1                # the explicit start, velocity "difference"
    assert dict(calls)["pdsolve_carry"] == (None,)
    its = [a for n, a in calls if n == "pdsolve_iterate"]
    assert all(a[0] == 3 and a[1] == 16 and a[3] is False for a in its)
    # steps 2 and 4 land in their slices of the records, the last step in q, the others nowhere
    step = records.stride(0) * records.element_size()
    assert [a[2] for a in its] == [None, records.data_ptr(), None, records.data_ptr() + step, q.data_ptr()]
    assert dict(calls)["pdsolve_positions"] == (q_prev.data_ptr(),)
    # the hyper-reduced path; the last step is a recorded one: q is its record
    for hyper in ("touched", "all"):
        calls, out = _rollout_calls(monkeypatch, lambda s: s.simulate_frames([red], 0.5, 3, num_iterations=2, velocity="zero", hyper=hyper,
                                                                             record_every=1))
        assert names(calls) == ["gstep_held", "gstep_setup", "rforce_operator", "hyper_operator", "pdsolve_begin", "pdsolve_carry",
                                "cproj_setup", "rforce_solver", "pdsolve_slot", "hyper_iterate", "pdsolve_advance", "hyper_iterate",
                                "pdsolve_advance", "hyper_iterate", "pdsolve_positions"]
        q, q_prev, nF, (records, steps) = out
        assert steps == [1, 2, 3] and q.data_ptr() == records[2].data_ptr()
        its = [a for n, a in calls if n == "hyper_iterate"]
        assert [a[3] for a in its] == [records[j].data_ptr() for j in range(3)]
        assert all((a[1] is None) == (hyper == "all") for a in its)
    # one step: no advance at all
    calls, out = _rollout_calls(monkeypatch, lambda s: s.simulate_frames([edge], 0.5, 1))
    assert names(calls) == ["gstep_held", "gstep_setup", "pdsolve_begin", "pdsolve_carry", "cproj_setup", "pdsolve_slot", "pdsolve_iterate",
                            "pdsolve_positions"] and len(out) == 3


def test_engine_calls_of_reduced_rollout_errors(monkeypatch):
    from test_dynamics_trace_cpu import _inputs, _reduced_kw
    c = _inputs()[0]
    for hyper in (None, "touched"):
        calls, out = _rollout_calls(monkeypatch, lambda s: s.reduced_rollout_errors("tets_strain", c.basis, [2, 4, 3], 0.5, 4, num_iterations=2,
                                                                                    record_every=2, hyper=hyper, **_reduced_kw()))
        names = [n for n, _ in calls]
        it = "pdsolve_iterate" if hyper is None else "hyper_iterate"
        roll = lambda i, solver: ["pdsolve_begin", "pdsolve_carry", "cproj_setup"] + solver + ["pdsolve_slot"] \
            + 3 * [i, "pdsolve_advance"] + [i, "pdsolve_positions"]
        assert names == ["gstep_held", "gstep_setup"] + roll("pdsolve_iterate", []) + ["rforce_operator"] + (["hyper_operator"] if hyper else []) \
            + 3 * (roll(it, ["rforce_solver"]) + 2 * ["force_diff"])
        assert out[5] == [2, 4] and all(a.shape == (3, 2) for a in out[:5])
    calls, out = _rollout_calls(monkeypatch, lambda s: s.reduced_rollout_errors("tets_strain", c.basis, [], 0.5, 4, **_reduced_kw()))
    assert calls == [] and out[5] == [1, 2, 3, 4] and all(a.shape == (0, 4) for a in out[:5])


def test_new_abi_names_are_declared():
    for name in ("asb_pdsolve_carry", "asb_pdsolve_advance", "asb_pdsolve_positions", "asb_test_pdsolve_state"):
        assert name in _lib.PROTOTYPES
        assert hasattr(_lib.load(), name)
