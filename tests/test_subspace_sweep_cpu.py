"""CPU: ``subspace_rollout_errors`` and ``subspace_distance`` (animsnapbases_amd/dynamics.py) on the recording
double of tests/test_dynamics_trace_cpu.py -- the engine calls of the sweep (one baseline roll-out, then per r one set-up, one
roll-out in z and exactly R fused comparisons; never ``gsub_expand`` or ``force_diff``), the empty sweep, every refusal with no
engine call recorded, what ``baseline="full"`` hands the engine, and the selected solver on every way out.  Every test fails on the
parent commit, where the two methods do not exist."""
import numpy as np
import pytest

from test_dynamics_trace_cpu import RecordingEngine, _bare, _inputs, _kinds

ZRUN = ["rforce_operator", "zroll_operator", "zroll_begin", "cproj_setup", "rforce_solver", "zroll_slot", "zroll_steps", "zroll_state"]
SUMS, MAXE, NORMS = np.array([1.0, 4.0, 9.0]), 2.0, np.array([4.0, 4.0, 4.0, 8.0])


class _Eng(RecordingEngine):
    """Answers what the sweep reads back: the set-ups' residuals and the records of the fused comparison."""
    def _gsub_setup(self, A, Qt, origin):
        return 0.25

    def _gsub_held(self, A, Qt, origin):
        return None

    def _gslab_setup(self, A, plan):
        return 0.0, (len(plan.slab_ptr) - 1, int(np.diff(plan.slab_ptr).max()))

    def _gsub_expand_diff(self, a, z, n_frames, per_frame=False):
        return SUMS.copy(), MAXE, NORMS.copy(), (np.full((n_frames, 2), 4.0) if per_frame else None)


def _spec(**kw):
    c = _inputs()[0]
    return dict(_kinds()[0], basis=c.basis, num_components=4, reduction=c.reduction, **kw)


def _comps(n):
    return np.random.default_rng(23).standard_normal((8, n, 3))


def _patched(monkeypatch):
    import torch
    real = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **kw: real(*a, **kw))
    eng = _Eng()
    return eng, _bare(eng)


def _names(eng):
    return [c[0] for c in eng.calls]


def test_engine_calls_of_the_sweep(monkeypatch):
    eng, snaps = _patched(monkeypatch)
    comps = _comps(snaps.nVerts)
    T, every, rs = 5, 2, [4, 8, 3]
    out = snaps.subspace_rollout_errors([_spec()], comps, rs, 0.5, T, 2, frame_start=1, frame_jump=2, record_every=every)
    fro, mx, rx, ry, rz, steps = out
    R = 2
    assert steps == [2, 4]
    for a in (fro, mx, rx, ry, rz):
        assert a.shape == (len(rs), R)
    # the arithmetic of _diff_metrics on the double's record
    assert (fro == np.sqrt(14.0)).all() and (mx == 0.25).all() and (rx == 0.5).all() and (ry == 1.0).all() and (rz == 1.5).all()
    names = _names(eng)
    first = names.index("gsub_held")
    base, rest = names[:first], names[first:]
    # one baseline roll-out with records: the hyper-reduced one under the explicit inverse
    assert base[:4] == ["gstep_held", "gstep_setup", "rforce_operator", "hyper_operator"]
    assert base.count("pdsolve_begin") == 1 and base.count("hyper_iterate") == T and base.count("pdsolve_advance") == T - 1
    assert base[-1] == "pdsolve_positions" and "pdsolve_iterate" not in base
    # then per r: one set-up, one roll-out in z, R comparisons
    assert rest == (["gsub_held", "gsub_setup"] + ZRUN + ["gsub_expand_diff"] * R) * len(rs)
    assert "gsub_expand" not in names and "force_diff" not in names
    for c in eng.calls:
        if c[0] == "zroll_steps":
            assert c[1][:4] == [T, 2, 0, every]
        if c[0] == "gsub_expand_diff":
            assert c[1][2] == len(range(1, snaps.frs, 2))
    # the subspaces handed over: r components each, in the order of r_values
    assert [c[1][1][0][1] for c in eng.calls if c[0] == "gsub_setup"] == rs
    # the selected solver is as before (none was selected)
    assert not hasattr(snaps, "_global_solver") and getattr(snaps, "_global_subspace", None) is None


def test_an_empty_sweep_touches_no_engine(monkeypatch):
    eng, snaps = _patched(monkeypatch)
    out = snaps.subspace_rollout_errors([_spec()], _comps(snaps.nVerts), [], 0.5, 5, 2, record_every=2)
    assert out[5] == [2, 4] and all(a.shape == (0, 2) for a in out[:5])
    assert eng.calls == []


def test_refusals_touch_no_engine(monkeypatch):
    import torch
    eng, snaps = _patched(monkeypatch)
    N, F = snaps.nVerts, snaps.frs
    comps = _comps(N)
    spec, plain = _spec(), _kinds()[0]
    sweep = lambda kinds=(spec,), basis=comps, rs=(4,), dt=0.5, T=3, **kw: snaps.subspace_rollout_errors(list(kinds), basis, list(rs), dt, T, 2, **kw)
    for rs in ([4, 0], [N + 1], [2.5], [True], [4, 9]):                                        # every r, also the last (9 > K = 8)
        with pytest.raises(ValueError, match="subspace_rollout_errors"):
            sweep(rs=rs)
    with pytest.raises(ValueError, match="subspace_rollout_errors.*needs a basis"):
        sweep(basis=None)
    for kinds in ([plain], [spec, plain], []):
        with pytest.raises(ValueError, match="subspace_rollout_errors: every kind must be reduced"):
            sweep(kinds=kinds)
    with pytest.raises(ValueError, match="every kind must be reduced"):
        snaps.subspace_rollout_errors(None, comps, [4], 0.5, 3)
    with pytest.raises(ValueError):                                                            # the engine holds one reduced operator
        sweep(kinds=[spec, dict(spec, kind="tets_deformation_gradient")])
    for every in (None, 0, 2.5):
        with pytest.raises(ValueError, match="record_every"):
            sweep(record_every=every)
    for bad in ("both", None, "Reduced", 1):
        with pytest.raises(ValueError, match="baseline must be 'reduced' or 'full'"):
            sweep(baseline=bad)
    for bad in (dict(T=0), dict(T=2.5), dict(dt=-1.0), dict(velocity="fast"), dict(gravity=(0.0, 1.0)), dict(frame_jump=0),
                dict(origin=np.zeros((N, 2)))):
        with pytest.raises(ValueError):
            sweep(**bad)
    with pytest.raises(ValueError, match="num_iterations"):
        snaps.subspace_rollout_errors([spec], comps, [4], 0.5, 3, 0)
    # the rows of the pins' shift and of the forces for num_steps steps; the force limit of a roll-out in z
    pins = dict(vertices=[0, 3], wi=1.0, shift=np.zeros((F + 1, 3)))
    with pytest.raises(ValueError, match="subspace_rollout_errors: pins: row %d of shift is needed" % (F + 1)):
        sweep(pins=pins)
    with pytest.raises(ValueError, match="subspace_rollout_errors: forces: row %d of force is needed" % (F + 1)):
        sweep(forces=dict(force=np.zeros((F + 1, N, 3))))
    with pytest.raises(ValueError, match="65536 rows of force, at most 65535"):
        sweep(forces=dict(force=np.zeros((65536, 2, 3)), vertices=[0, 3]))
    with pytest.raises(TypeError):                                                             # floor is not an argument
        sweep(floor=dict(height=0.0))
    # under the subspace itself: the message of subspace_solve_errors
    snaps.set_global_solver("subspace", basis=comps, num_components=4)
    with pytest.raises(ValueError, match="subspace_rollout_errors: the full solve runs under 'inverse' or 'slab'"):
        sweep()
    # subspace_distance: a subspace on the device, then both tensors, F' included
    x, z = torch.zeros((5, N, 3), dtype=torch.float64), torch.zeros((5, 4, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match="subspace_distance: no position subspace on the device"):
        snaps.subspace_distance(x, z)
    snaps.set_global_solver("inverse")
    with pytest.raises(ValueError, match="subspace_distance: no position subspace on the device"):
        snaps.subspace_distance(x, z)
    snaps._comm.multi = True
    for call in (sweep, lambda: snaps.subspace_distance(x, z)):
        with pytest.raises(NotImplementedError, match="several ranks"):
            call()
    assert eng.calls == []


def test_subspace_distance_checks_both_tensors_before_the_engine(monkeypatch):
    import torch
    eng, snaps = _patched(monkeypatch)
    N = snaps.nVerts
    snaps.set_global_solver("subspace", basis=_comps(N), num_components=4)
    snaps.global_solve_setup([_kinds()[0]], 0.5)
    del eng.calls[:]
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: type("S", (), {"synchronize": lambda self: None})())
    monkeypatch.setattr(type(eng), "device_id", None)                                         # (a host tensor's device index)
    x, z = torch.zeros((5, N, 3), dtype=torch.float64), torch.zeros((5, 4, 3), dtype=torch.float64)
    for bx, bz in ((x.float(), z), (x, z.float()), (x[:, :5], z), (x, z[:, :3]), (x, z[:4]), (x.transpose(0, 1), z), (x, "z"), (None, z)):
        with pytest.raises(ValueError, match="subspace_distance"):
            snaps.subspace_distance(bx, bz)
    assert eng.calls == []
    out = snaps.subspace_distance(x, z)
    assert out == (np.sqrt(14.0), 0.25, 0.5, 1.0, 1.5)
    out = snaps.subspace_distance(x, z, per_frame=True)
    assert out[:5] == (np.sqrt(14.0), 0.25, 0.5, 1.0, 1.5) and out[5].shape == (5,) and (out[5] == 1.0).all()
    assert _names(eng) == ["gsub_expand_diff"] * 2 and [c[1][2:] for c in eng.calls] == [[5, False], [5, True]]


def test_the_full_baseline_strips_the_reduction(monkeypatch):
    """``pdsolve_slot`` receives S^T (its third argument) for every kind under ``baseline="full"`` and None for the reduced kind
    under "reduced"; the roll-outs in z are the same calls under both."""
    got = {}
    for baseline in ("reduced", "full"):
        eng, snaps = _patched(monkeypatch)
        snaps.subspace_rollout_errors([_spec()], _comps(snaps.nVerts), [4], 0.5, 3, 2, baseline=baseline)
        names = _names(eng)
        first = names.index("gsub_held")
        slots = [c[1][2] for c in eng.calls[:first] if c[0] == "pdsolve_slot"]
        assert len(slots) == 1
        got[baseline] = (slots[0], names[:first], names[first:])
    assert got["reduced"][0] is None and "csr" in got["full"][0]
    assert "hyper_iterate" in got["reduced"][1] and "pdsolve_iterate" not in got["reduced"][1]
    assert got["full"][1].count("pdsolve_iterate") == 3 and not any(n.startswith(("hyper_", "rforce_")) for n in got["full"][1])
    assert got["full"][2] == got["reduced"][2]


def test_the_selected_solver_is_restored_on_every_way_out(monkeypatch):
    eng, snaps = _patched(monkeypatch)
    comps = _comps(snaps.nVerts)
    run = lambda: snaps.subspace_rollout_errors([_spec()], comps, [4, 8], 0.5, 3, 2)

    def boom(*a, **k):
        raise RuntimeError("engine")
    # none selected: none afterwards
    run()
    assert not hasattr(snaps, "_global_solver") and getattr(snaps, "_global_subspace", None) is None
    eng._zroll_steps = boom
    with pytest.raises(RuntimeError, match="engine"):
        run()
    assert not hasattr(snaps, "_global_solver") and getattr(snaps, "_global_subspace", None) is None
    # the slab solver: the baseline runs under it, and it is in force afterwards -- also when the second r fails
    snaps.set_global_solver("slab", slab_target=8)
    del eng._zroll_steps
    del eng.calls[:]
    run()
    assert snaps._global_solver == ("slab", 8) and snaps._global_subspace is None
    assert _names(eng)[:2] == ["gslab_held", "gslab_setup"] and "gstep_setup" not in _names(eng)
    count = {"n": 0}

    def second(*a, **k):
        count["n"] += 1
        if count["n"] == 2:
            raise RuntimeError("engine")
    eng._zroll_steps = second
    with pytest.raises(RuntimeError, match="engine"):
        run()
    assert count["n"] == 2 and snaps._global_solver == ("slab", 8) and snaps._global_subspace is None
    # a refusal from inside a roll-out in z: a ValueError leaves the same state
    del eng._zroll_steps

    def refuse(*a, **k):
        raise ValueError("inside")
    eng._zroll_begin = refuse
    with pytest.raises(ValueError, match="inside"):
        run()
    assert snaps._global_solver == ("slab", 8) and snaps._global_subspace is None


def test_the_symbol_is_declared_and_bound():
    import os
    import re
    from animsnapbases_amd import _lib
    assert len(_lib.PROTOTYPES["asb_gsub_expand_diff"][1]) == 8
    here = os.path.dirname(os.path.abspath(__file__))
    header = open(os.path.join(here, "..", "include", "asb.h")).read()
    assert re.search(r"int asb_gsub_expand_diff\(asb_ctx\* ctx, const double\* a_dev, const double\* z_dev, int64_t n_frames", header)
    from animsnapbases_amd.engine import HipEngine
    import inspect
    sig = inspect.signature(HipEngine.gsub_expand_diff)
    assert list(sig.parameters) == ["self", "a_dev_ptr", "z_dev_ptr", "n_frames", "per_frame"] and sig.parameters["per_frame"].default is False
