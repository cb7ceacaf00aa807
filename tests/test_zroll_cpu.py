"""CPU: the host side of the roll-outs whose state lives in z -- the defining properties of the longdouble model
of tests/zroll_model.py, the refusals and the engine calls of ``simulate_subspace`` / ``subspace_coordinates`` / ``subspace_expand``
on a recording double, and the facts about the fixtures that tests/zroll_cases.py relies on.

Measured here (this model, no device): against ``rollout_cases.rollout`` under the Galerkin case on frames inside o + span(U) the
first step agrees to 2.0e-16 .. 3.4e-16 relative; the later steps of the float64 roll-out carry its own roundings amplified
(amp up to 33) and reach 2.3e-15 at tets_deim r = 8, step 2 -- they are printed, and held to 4 eps max(1, amp_t) t.
Amplification: tris_blocks <= 7.5 (pinned <= 7.9), tets_deim rows of ``TETS_ROWS`` <= 32.6, pinned tets_deim (r = 4) <= 43.8."""
import numpy as np
import pytest

import rollout_cases as rc
import zroll_cases as zc
from gsub_model import EPS
from test_gsub_cpu import _Recorder, _bare
from zroll_model import ZModel


# ------------------------------------------------------------------ the host model
@pytest.mark.parametrize("fixture,r,m,K,T", zc.FREE)
def test_model_equals_the_subspace_rollout_on_frames_in_the_span(fixture, r, m, K, T):
    """For x_f, x_{f-1} in o + span(U) the recurrence in z IS ``simulate_frames(hyper=)`` under the subspace: the longdouble model
    against the float64 ``rollout_cases.rollout`` whose ``lu`` is the Galerkin map.  Step 1 to 1e-15 relative.  From step 2 on
    the float64 roll-out's own roundings (eps / 2 per iterate and per carry, a few per step) have passed through its later
    steps, which ``amp`` measures: 4 eps max(1, amp_t) t."""
    s = zc.z_case(fixture, r)
    op = zc.operator(s, m)
    zm = ZModel(s, {0: op})
    c = dict(s, frames=s["proj_frames"])
    for mode in zc.MODES:
        s0, p0 = rc.start_state(c["frames"], zc.SEL, mode)
        host = rc.rollout(c, K, T, s0, p0, reduced=(0, op))
        zs, _ = zm.rollout(*zm.start(c["frames"], zc.SEL, mode), K, T)
        amp = zc.amp_of(s, m, mode, K, T)
        rel = [float(np.abs(zm.expand(zs[t]).astype(np.float64) - host[t]).max() / np.abs(host[t]).max()) for t in range(T)]
        print("%s r = %d m = %d K = %d %s: relative difference per step %s" % (fixture, r, m, K, mode, ["%.2g" % x for x in rel]))
        assert rel[0] <= 1e-15
        for t in range(1, T):
            assert rel[t] <= 4 * EPS * max(1.0, amp[t]) * (t + 1)


@pytest.mark.parametrize("fixture,m", [("tris_blocks", 8), ("tets_deim", 17)])
def test_the_full_basis_is_the_full_hyper_reduced_rollout(fixture, m):
    """r = N: U^T A U is similar to A, the Galerkin step is A^-1, every frame lies in the span: the model equals the float64
    roll-out with the sparse LU from any start.  Held to what that roll-out itself commits: per iteration 64 eps kappa(A) max |q|
    (the LU solve) through ``bound_T`` with the amplification measured on it."""
    import pdsolve_cases as pc
    s = zc.z_case(fixture, None)
    full = pc.host_case(s["rf"].kind)
    op = zc.operator(s, m)
    zm = ZModel(s, {0: op})
    K, T = 3, 2
    kappa = float(np.linalg.cond(full["A"].toarray()))
    for mode in zc.MODES:
        s0, p0 = rc.start_state(full["frames"], zc.SEL, mode)
        host = rc.rollout(full, K, T, s0, p0, reduced=(0, op))
        zs, recs = zm.rollout(*zm.start(full["frames"], zc.SEL, mode), K, T)
        amp = rc.measure_amp(full, mode, K, T, zc.SEL, reduced=(0, op))
        for t in range(T):
            one = 64 * EPS * kappa * float(np.abs(host[t]).max())
            B = rc.bound_T(one, K, t + 1, float(amp[t]), rc.adv_bound(host[t], host[t]))
            err = float(np.abs(zm.expand(zs[t]).astype(np.float64) - host[t]).max())
            print("%s r = N %s step %d: |model - full| %.3g, bound %.3g" % (fixture, mode, t + 1, err, B))
            assert err <= B
    # the projection of a frame onto the full basis is the frame
    x = full["frames"][zc.SEL]
    assert np.abs(zm.project(x) - x).max() <= (zm.g.N + 2) * EPS * np.abs(x).max() * 2


def test_coordinates_and_expansion_are_inverse_on_the_span():
    s = zc.z_case("tris_blocks", 8)
    zm = ZModel(s, {0: zc.operator(s, 3)})
    z = np.random.default_rng(2).standard_normal((5, 8, 3))
    back = zm.coordinates(zm.expand(z).astype(np.float64)).astype(np.float64)
    assert np.abs(back - z).max() <= 3 * zc.start_bound(zm, zm.expand(z).astype(np.float64)) + 64 * EPS


# ------------------------------------------------------------------ the fixtures
@pytest.mark.parametrize("fixture,r,m,K,T", zc.FREE)
def test_the_unpinned_cases_are_suitable(fixture, r, m, K, T):
    s = zc.z_case(fixture, r)
    for mode in zc.MODES:
        amp = zc.amp_of(s, m, mode, K, T)
        print("%s r = %d m = %d K = %d T = %d %s: amp %s" % (fixture, r, m, K, T, mode, np.array2string(amp, precision=1)))
        assert amp.shape == (T,) and amp[-1] <= zc.AMP_CAP
        assert amp[-1] <= (7.6 if fixture == "tris_blocks" else 33.0)          # what the issue's table states for these rows


@pytest.mark.parametrize("fixture,pn,r,m,K,T", zc.PINNED)
def test_the_pinned_cases_are_suitable(fixture, pn, r, m, K, T):
    import pins_cases as pins
    s = zc.z_case(fixture, r, pn)
    acc = s["dt"] ** 2 * np.array(pins.G)
    assert s["pins"][0].tolist() == list(zc.PIN_SETS[pn]["vertices"]) and (s["pins"][3] is not None) == zc.PIN_SETS[pn]["moving"]
    for mode in zc.MODES:
        amp = zc.amp_of(s, m, mode, K, T, acc)
        print("%s %s r = %d m = %d K = %d T = %d %s: amp %s" % (fixture, pn, r, m, K, T, mode, np.array2string(amp, precision=1)))
        assert amp[-1] <= zc.AMP_CAP and amp[-1] <= (8.0 if fixture == "tris_blocks" else 154.0)


def test_the_excluded_row_exceeds_the_cap():
    """tets_deim r = 8, K = 3, T = 5 is not run: its amplification is above AMP_CAP (why ``TETS_ROWS`` stops at T = 2 for r = 8)."""
    s = zc.z_case("tets_deim", 8)
    amp = max(float(zc.amp_of(s, 17, mode, 3, 5)[-1]) for mode in zc.MODES)
    print("tets_deim r = 8 K = 3 T = 5: amp %.3g" % amp)
    assert amp > zc.AMP_CAP and ("tets_deim", 8, 17, 3, 5) not in zc.FREE


# ------------------------------------------------------------------ the public methods on a recording double
class _Rec(_Recorder):
    def _gsub_setup(self, A, Qt, origin):
        self.held = (A.data.copy(), Qt.copy(), origin.copy())
        return 0.25


def _reduced_spec(kind):
    c = __import__("reduced_forces_cases").case("tets_deim")
    return dict(kind, basis=c.basis, num_components=c.ms[0], reduction=c.reduction)


def test_refusals_touch_no_engine():
    import torch
    eng = _Rec()
    snaps, kind, comps = _bare(eng)
    spec = _reduced_spec(kind)
    # no subspace in force
    with pytest.raises(ValueError, match="simulate_subspace.*set_global_solver"):
        snaps.simulate_subspace([spec], 0.5, 2)
    with pytest.raises(ValueError, match="subspace_coordinates: no position subspace"):
        snaps.subspace_coordinates("train")
    with pytest.raises(ValueError, match="subspace_expand: no position subspace"):
        snaps.subspace_expand(torch.zeros((2, 4, 3), dtype=torch.float64))
    snaps.set_global_solver("subspace", basis=comps, num_components=4)
    with pytest.raises(ValueError, match="subspace_coordinates: no position subspace"):        # selected, but not set up on the device
        snaps.subspace_coordinates("train")
    # a plain kind, alone or beside a reduced one
    for kinds in ([kind], [spec, kind], [], None):
        with pytest.raises(ValueError, match="every kind must be reduced"):
            snaps.simulate_subspace(kinds, 0.5, 2)
    with pytest.raises(ValueError, match="second reduced kind"):                               # the limit of set_reduced_kinds
        snaps.simulate_subspace([spec, dict(spec, kind="tets_deformation_gradient")], 0.5, 2)
    # the state: a pair of float64 device tensors (F', r, 3)
    host = torch.zeros((snaps.frs, 4, 3), dtype=torch.float64)
    for state in (host, (host,), (host, host), (host.float(), host.float()), "z"):
        with pytest.raises(ValueError, match="state"):
            snaps.simulate_subspace([spec], 0.5, 2, state=state)
    # the roll-out's own arguments, the pins' rows
    for bad in (dict(num_steps=0), dict(num_steps=2.5), dict(num_steps=2, record_every=0), dict(num_steps=2, num_iterations=0),
                dict(num_steps=2, velocity="fast"), dict(num_steps=2, dt=-1.0)):
        kw = dict(dt=0.5)
        kw.update(bad)
        with pytest.raises(ValueError):
            snaps.simulate_subspace([spec], **kw)
    pins = dict(vertices=[0, 3], wi=1.0, shift=np.zeros((snaps.frs + 1, 3)))
    with pytest.raises(ValueError, match="row %d of shift is needed" % (snaps.frs + 1)):
        snaps.simulate_subspace([spec], 0.5, 3, pins=pins)
    snaps._comm.multi = True
    for call in (lambda: snaps.simulate_subspace([spec], 0.5, 2), lambda: snaps.subspace_coordinates("train"), lambda: snaps.subspace_expand(host)):
        with pytest.raises(NotImplementedError, match="several ranks"):
            call()
    assert eng.calls == []


def test_engine_calls_of_a_rollout_in_z(monkeypatch):
    import torch
    real = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **kw: real(*a, **kw))
    eng = _Rec()
    snaps, kind, comps = _bare(eng)
    spec = _reduced_spec(kind)
    snaps.set_global_solver("subspace", basis=comps, num_components=4)
    out = snaps.simulate_subspace([spec], 0.5, 3, 2, record_every=1)
    run = ["rforce_operator", "zroll_operator", "zroll_begin", "cproj_setup", "rforce_solver", "zroll_slot", "zroll_steps", "zroll_state"]
    assert eng.calls == ["gsub_held", "gsub_setup"] + run
    z, z_prev, nF, (records, steps) = out
    assert nF == snaps.frs and tuple(z.shape) == tuple(z_prev.shape) == (nF, 4, 3) and tuple(records.shape) == (3, nF, 4, 3) and steps == [1, 2, 3]
    assert not any(c.startswith(("hyper_", "pdsolve_", "gstep_run")) for c in eng.calls)
    # held; pins: set before the begin, bound behind it; the operators once, one zroll_steps whatever T is
    del eng.calls[:]
    pins = dict(vertices=[0, 3], wi=[0.7, 10.0])
    snaps.simulate_subspace([spec], 0.5, 7, 2, pins=pins)
    assert eng.calls == ["gsub_held", "gsub_setup", "rforce_operator", "zroll_operator", "pins_set", "zroll_begin", "zroll_pins", "cproj_setup",
                         "rforce_solver", "zroll_slot", "zroll_steps", "zroll_state"]
    assert list(snaps.assembly_ST) == ["tets_strain", "positional"]
    # coordinates and expansion need the set-up, then one call each
    del eng.calls[:]
    assert tuple(snaps.subspace_coordinates("train", 2, 9, 2).shape) == (4, 4, 3)
    assert eng.calls == ["gsub_coordinates"]
    # two reduced kinds: banks 0 and 1, bank 0 current again at the end -- also when the engine fails
    snaps.set_reduced_kinds(2)
    two = [spec, dict(spec, kind="tets_deformation_gradient")]
    del eng.calls[:]
    snaps.simulate_subspace(two, 0.5, 2, 2)
    assert eng.calls == ["gsub_held", "gsub_setup", "rforce_bank", "rforce_operator", "zroll_operator", "rforce_bank", "rforce_operator",
                         "zroll_operator", "zroll_begin", "rforce_bank", "cproj_setup", "rforce_solver", "zroll_slot", "rforce_bank", "cproj_setup",
                         "rforce_solver", "zroll_slot", "zroll_steps", "zroll_state", "rforce_bank"]

    def boom(*a, **k):
        raise RuntimeError("engine")
    eng._zroll_steps = boom
    del eng.calls[:]
    with pytest.raises(RuntimeError, match="engine"):
        snaps.simulate_subspace(two, 0.5, 2, 2)
    assert eng.calls[-2:] == ["zroll_steps", "rforce_bank"]
