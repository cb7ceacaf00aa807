"""GPU (-m gpu): positional constraints (pins) in the resident solver -- asb_pins_set / asb_pins_term / asb_fm_add / asb_pdsolve_pins
and the pin launch of asb_pdsolve_advance (csrc/asb_pdsolve.hip), and ``pins=`` of posSnapshots.constraint_forces / global_step /
solve_frames / simulate_frames and the error sweeps -- against the fixtures of the UNMODIFIED reference's
``step()`` with its ``PositionalConstraint`` objects (tools/gen_golden_pins.py), against the host route of tests/pins_cases.py for
the reduced kind, step by step against one NumPy iteration from the device's OWN two previous records, and bit for bit against
``global_step``, ``solve_frames`` and itself.

Shapes.  k_pins_fm's block is 4 pins x 64 frames: chains of N in {2, 15, 16, 17, 31, 32, 33, 65} at F' in {1, 63, 64, 65, 130} with
pins on {0}, {N - 1}, {0, N - 1} and all N vertices (P = 1, 2 and N: less than a block of pins, whole blocks, a ragged last one),
fixed, with a shared (T_s, 3) shift and with a per-pin (T_s, P, 3) shift; and the goldens (N = 18, 42; F' = 44).

Bounds: tests/pins_cases.py -- B of rollout_cases with the one-iteration bound extended by the pin term's three roundings; amp
measured on the host model and stored with the fixtures.  No start frame is left out.  Every error is printed beside its bound."""
import contextlib
import io

import numpy as np
import pytest

import pins_cases as pins
from conftest import load_golden
from gstep_cases import EPS, golden
from hyper_cases import one_bound as hyper_one_bound
from pdsolve_cases import AMP_CAP, KS, MODES, host_case, parts_of
from reduced_forces_cases import case as rf_case, operator as rf_operator
from rollout_cases import START_FRAMES, adv_bound, bound_T, start_state
from test_gpu_cforces import _bound as force_bound, _g
from test_gpu_cproj import RAW_TOL, _kappa, _min_edge
from test_gpu_gstep import _case, _report
from test_gpu_pdsolve import _mesh, _reduced_kw, _snaps
from test_gpu_rollout import _chain_bound, _chain_case, _dev, _prev
from test_pins_cpu import kinds_force_bound

pytestmark = pytest.mark.gpu

CHAINS = [2, 15, 16, 17, 31, 32, 33, 65]
FRAMES = [1, 63, 64, 65, 130]
SEL = dict(frame_jump=3)                                            # range(0, 130, 3): START_FRAMES
G = pins.G


def _rest(name):
    return load_golden("cproj_" + parts_of(pins.FIXTURES[name]["base"])[-1])["rest"]


# ------------------------------------------------------------------ 1. against the reference's steps with its PositionalConstraint
def _against_reference(name, snaps, tol_p, tag):
    fx = pins.FIXTURES[name]
    zg, frames, kinds, _ = _case(fx["base"], tol_p)
    z, c = load_golden("pins_" + name), pins.host_case(name)
    dt, masses = float(zg["dt"]), zg["masses"]
    P = pins.pins_of(name, _rest(name))
    fb = kinds_force_bound(name, tol_p)
    acc = dt * dt * np.array(G)
    steps = z["steps"].tolist()
    T = max(steps)
    kw = dict(gravity=G, **SEL)
    stiff = int(np.argmax(P["wi"]))                                 # the pin of weight 1e3
    worst = 0.0
    for mode in MODES:
        # global_step: one iteration from the frame
        ref = z["g_" + mode]
        B = 2.0 * pins.one_bound(c, fb, np.abs(ref).max(), START_FRAMES)
        step, nF = snaps.global_step(kinds, dt, masses, velocity=mode, pins=P, **kw)
        assert nF == len(START_FRAMES)
        err = _report("%s %s global_step %s" % (name, mode, tag), step.cpu().numpy(), ref, B)
        assert err <= B
        worst = max(worst, err / B)
        free = snaps.global_step(kinds, dt, masses, velocity=mode, **kw)[0]
        assert np.abs(free.cpu().numpy() - step.cpu().numpy()).max() > B         # the pins matter
        for K in KS:
            bound = lambda t, ref: bound_T(pins.one_bound(c, fb, np.abs(ref).max(), START_FRAMES), K, t,
                                           float(z["amp_%s_%d_%d" % (mode, K, t)]), adv_bound(ref, ref, acc))
            # solve_frames: the fixture's first step
            ref = z["q_%s_%d_1" % (mode, K)]
            B = bound(1, ref)
            out = snaps.solve_frames(kinds, dt, K, masses, velocity=mode, pins=P, **kw)[0]
            err = _report("%s %s K = %d solve_frames %s" % (name, mode, K, tag), out.cpu().numpy(), ref, B)
            assert err <= B
            worst = max(worst, err / B)
            # simulate_frames: every kept step
            q, q_prev, nF, (rec, rsteps) = snaps.simulate_frames(kinds, dt, T, K, masses, velocity=mode, record_every=1, pins=P, **kw)
            assert nF == len(START_FRAMES) and rsteps == list(range(1, T + 1))
            assert list(snaps.assembly_ST) == [k["kind"] for k in kinds] + ["positional"]
            got = rec.cpu().numpy()
            for t in steps:
                ref = z["q_%s_%d_%d" % (mode, K, t)]
                B = bound(t, ref)
                err = _report("%s %s K = %d T = %d %s" % (name, mode, K, t, tag), got[t - 1], ref, B)
                assert err <= B
                worst = max(worst, err / B)
            # without pins the roll-out is somewhere else, by more than the bound
            loose = snaps.simulate_frames(kinds, dt, T, K, masses, velocity=mode, **kw)[0].cpu().numpy()
            assert np.abs(loose - got[T - 1]).max() > B
            if K == 10:
                # the stiffly pinned vertex stays as near its target as the host model says; the unpinned run has fallen
                host = pins.rollout(c, K, T, *start_state(frames, START_FRAMES, mode, acc), START_FRAMES, acc)[T - 1]
                v = P["vertices"][stiff]
                target = pins.targets(c, np.array(START_FRAMES) + T - 1)[:, stiff]
                d_host = np.abs(host[:, v] - target).max()
                d_dev, d_free = np.abs(got[T - 1][:, v] - target).max(), np.abs(loose[:, v] - target).max()
                print("%s %s T = %d: pinned vertex %d off its target by %.3g (host model %.3g), unpinned run by %.3g"
                      % (name, mode, T, v, d_dev, d_host, d_free))
                assert d_dev <= d_host + B and d_free > d_host + B and d_free > 10.0 * d_dev
    print("%s %s: largest err / B %.3g" % (name, tag, worst))


@pytest.mark.parametrize("name", sorted(pins.FIXTURES))
def test_pinned_steps_match_the_reference(name):
    frames = _case(pins.FIXTURES[name]["base"])[1]
    _against_reference(name, _snaps(frames), RAW_TOL, "raw")


@pytest.mark.parametrize("name", sorted(pins.FIXTURES))
def test_pinned_steps_on_a_weighted_standardised_tensor(name):
    kinds = parts_of(pins.FIXTURES[name]["base"])
    g = _g(kinds[-1])[0]
    tol_p = 64 * EPS * np.abs(g["frames"]).max() * max(_kappa(k, _g(k)[0]) / _min_edge(k, _g(k)[0]) for k in kinds)
    mass = 0.5 + np.random.default_rng(3).random(g["frames"].shape[1])         # the weighting of the tensor is not the solver's mass
    snaps = _snaps(g["frames"], standarize=True, mass=mass)
    assert snaps.pre_scale_factor != 1 and snaps.massL is not None
    _against_reference(name, snaps, tol_p, "weighted")


def test_pinned_steps_under_the_slab_solver_match_the_reference():
    name = "edge_spring_fixed"
    snaps = _snaps(_case(pins.FIXTURES[name]["base"])[1])
    snaps.set_global_solver("slab", 4)
    _against_reference(name, snaps, RAW_TOL, "slab")
    assert snaps.global_solve_slabs[0] > 1


def test_reduced_and_hyper_steps_with_pins_match_the_host_route():
    """The reduced side has no reference run: the device against the host route, plain and hyper-reduced; the amplification is
    measured here, on the host model."""
    c = rf_case("tris_blocks")
    z = golden(c.kind)
    frames, rest = c.g["frames"], c.g["rest"]
    N = frames.shape[1]
    dt, masses = float(z["dt"]), z["masses"]
    v = np.array([1, N // 2, N - 2])
    P = dict(vertices=v, wi=np.array([0.7, 1e3, 1.4]), positions=rest[v], shift=pins.shift_of(1)[:, 0], shift_start=2)
    hc = pins.with_pins(host_case(c.kind), P)
    ainv, kappa = pins.matrix_numbers(hc)
    acc = dt * dt * np.array(G)
    rows = np.array(START_FRAMES) + 2
    fb = force_bound(_g(c.kind)[2], c.g["expected"], RAW_TOL).max()
    snaps = _snaps(frames)
    m, T = c.ms[-1], 2
    op = rf_operator(c, m)
    spec = [dict(kind=c.kind, basis=c.basis, num_components=m, reduction=c.reduction, **_reduced_kw(c))]
    for mode in MODES:
        s, x = start_state(frames, START_FRAMES, mode, acc)
        for K in (1, 3):
            amp = pins.measure_amp(hc, mode, K, T, START_FRAMES, acc, reduced=(0, op))
            assert amp[-1] <= AMP_CAP
            host = pins.rollout(hc, K, T, s, x, rows, acc, reduced=(0, op))
            runs = {h: snaps.simulate_frames(spec, dt, T, K, masses, velocity=mode, gravity=G, record_every=1, hyper=h, pins=P, **SEL)
                    for h in (None, "touched", "all")}
            for t in (1, 2):
                one = hyper_one_bound(ainv, kappa, c.St, op, c.p_pt(m), c.r["cond_%d" % m], fb, RAW_TOL, np.abs(host[t - 1]).max()) \
                    + ainv * pins.pin_rounding(hc, rows)
                B = bound_T(one, K, t, float(amp[t - 1]), adv_bound(host[t - 1], host[t - 1], acc))
                for h, run in runs.items():
                    assert _report("tris_blocks m = %d %s K = %d T = %d hyper %s" % (m, mode, K, t, h), run[3][0][t - 1].cpu().numpy(),
                                   host[t - 1], B) <= B
            import torch
            assert torch.equal(runs["touched"][3][0], runs["all"][3][0]) and torch.equal(runs["touched"][1], runs["all"][1])
            loose = snaps.simulate_frames(spec, dt, T, K, masses, velocity=mode, gravity=G, hyper="touched", **SEL)[0]
            assert np.abs(loose.cpu().numpy() - host[T - 1]).max() > B
    # the sweeps take the pins along: one step of the roll-out sweep is the solve sweep, and both differ from the unpinned ones
    kw = dict(reduction=c.reduction, gravity=G, frame_jump=3, **_reduced_kw(c))
    for hyper in (None, "touched"):
        one = snaps.reduced_rollout_errors(c.kind, c.basis, [c.ms[0], m], dt, 1, 3, masses, record_every=1, hyper=hyper, pins=P, **kw)
        old = snaps.reduced_solve_errors(c.kind, c.basis, [c.ms[0], m], dt, 3, masses, hyper=hyper, pins=P, **kw)
        bare = snaps.reduced_solve_errors(c.kind, c.basis, [c.ms[0], m], dt, 3, masses, hyper=hyper, **kw)
        assert one[5] == [1] and all(one[j][:, 0].tolist() == old[j] for j in range(5)) and old[0] != bare[0]
    assert list(snaps.assembly_ST) == [c.kind]
    step = snaps.reduced_global_step_errors(c.kind, c.basis, [m], dt, masses, pins=P, **kw)
    bare = snaps.reduced_global_step_errors(c.kind, c.basis, [m], dt, masses, **kw)
    assert np.isfinite(step[0]).all() and step[0] != bare[0] and list(snaps.assembly_ST) == [c.kind]


# ------------------------------------------------------------------ 2. chains: every step against one host iteration of the device's own records
def _pin_sets(n, F):
    """(pins dict, tag) for the four vertex sets: fixed, a shared shift, a per-pin shift, and all N with a per-pin shift."""
    rows = F + 8
    rest = _chain_case(n)["spec"][0]["rest_positions"]
    sets = [([0], None), ([n - 1], pins.shift_of(1, rows)[:, 0])]
    if n > 1:
        sets.append(([0, n - 1], pins.shift_of(2, rows)))
    sets.append((list(range(n)), pins.shift_of(n, rows)))
    out = []
    for v, sh in sets:
        v = np.array(v)
        p = dict(vertices=v, wi=np.where(v % 2 == 0, 3.0, 1e3), positions=rest[v] + 0.01)
        if sh is not None:
            p.update(shift=sh, shift_start=2)
        out.append(p)
    return out


@pytest.mark.parametrize("n", CHAINS)
def test_every_pinned_step_is_one_host_iteration_from_the_devices_own_records(n):
    base = dict(_chain_case(n), wis=[_chain_case(n)["spec"][0]["wi"]])
    frames, dt = base["frames"], base["dt"]
    acc = dt * dt * np.array(G)
    snaps = _snaps(frames)
    T = 3
    for F in FRAMES:
        for i, P in enumerate(_pin_sets(n, F)):
            mode = MODES[(i + F) % 2]
            c = pins.with_pins(base, P)
            c["Ainv_abs_inf"], c["kappa"] = pins.matrix_numbers(c)
            rows = np.arange(F) + P.get("shift_start", 0)
            q, q_prev, nF, (rec, steps) = snaps.simulate_frames(c["spec"], dt, T, 1, c["masses"], velocity=mode, gravity=G, record_every=1,
                                                                frame_end=F, pins=P)
            assert nF == F and steps == [1, 2, 3]
            r = rec.cpu().numpy()
            assert np.isfinite(r).all()
            x = frames[:F]
            hist = [x if mode == "zero" else _prev(frames, range(F)), x] + list(r)
            worst = 0.0
            for t in range(1, T + 1):
                s = 2.0 * hist[t] - hist[t - 1] + acc[None, None, :]
                want = pins.iterate(c, s, s, 1, rows + t - 1)
                B = _chain_bound(c, s, want) + c["Ainv_abs_inf"] * pins.pin_rounding(c, rows + t - 1)
                err = np.abs(r[t - 1] - want).max()
                worst = max(worst, err / B)
                assert err <= B, (n, F, P["vertices"].tolist(), mode, t, err, B)
            # another row of the shift, or no pins at all, is further away than the bound
            if "shift" in P:
                assert np.abs(r[T - 1] - pins.iterate(c, s, s, 1, rows + T)).max() > B
            loose = snaps.simulate_frames(c["spec"], dt, T, 1, c["masses"], velocity=mode, gravity=G, frame_end=F)[0].cpu().numpy()
            assert np.abs(loose - r[T - 1]).max() > B
            print("chain %d F' = %d pins %d %s: largest err / bound %.3g (bound %.3g)" % (n, F, P["vertices"].size, mode, worst, B))


@pytest.mark.parametrize("n", [2, 17, 65])
def test_the_pin_term_kernel_writes_what_it_owns_and_nothing_else(n):
    """asb_pins_term alone: the host's wi (p0 + shift[row]) to the bit; a store writes +0.0 elsewhere, an accumulation leaves
    every other entry untouched; constraint_forces(pins=) is constraint_forces plus that term."""
    import torch
    frames, kinds, m, dt = _mesh("chain%d" % n)
    snaps = _snaps(frames)
    eng = snaps._engine
    for F in FRAMES:
        for P in _pin_sets(n, 2 * F):
            c = pins.with_pins(dict(_chain_case(n), wis=[kinds[0]["wi"]]), P)
            f0, fj = (0, 1) if F == 1 else (1, 2)
            sel = list(range(f0, F, fj))
            want = pins.pin_term(c, np.array(sel) + P.get("shift_start", 0))
            rec = snaps._pins("test", P)
            eng.pins_set(rec.vertices, rec.wi, rec.p0, rec.shift)
            out = torch.full((len(sel), n, 3), float("nan"), dtype=torch.float64, device="cuda:%d" % eng.device_id)
            torch.cuda.synchronize()
            eng.pins_term(f0, F, fj, rec.start, False, out.data_ptr())
            got = out.cpu().numpy()
            assert np.array_equal(got, want) and not np.signbit(got[want == 0.0]).any()
            base = torch.from_numpy(np.random.default_rng(n + F).standard_normal(want.shape)).to(out.device)
            base[:, [v for v in range(n) if v not in set(P["vertices"].tolist())]] = float("nan")
            acc = base.clone()
            torch.cuda.synchronize()
            eng.pins_term(f0, F, fj, rec.start, True, acc.data_ptr())
            b, a = base.cpu().numpy(), acc.cpu().numpy()
            pinned = np.zeros(n, dtype=bool)
            pinned[P["vertices"]] = True
            assert np.array_equal(a[:, pinned], b[:, pinned] + want[:, pinned]) and np.isnan(a[:, ~pinned]).all()
            eng.fm_add(acc.data_ptr(), out.data_ptr(), out.numel())
            assert np.array_equal(acc.cpu().numpy()[:, pinned], a[:, pinned] + want[:, pinned])
            plain = snaps.constraint_forces(kinds, frame_start=f0, frame_end=F, frame_jump=fj)[0].cpu().numpy()
            with_p, nF = snaps.constraint_forces(kinds, frame_start=f0, frame_end=F, frame_jump=fj, pins=P)
            assert nF == len(sel) and np.array_equal(with_p.cpu().numpy(), plain + want)
            assert list(snaps.assembly_ST) == ["edge_spring", "positional"] and snaps.assembly_ST["positional"].shape == (n, P["vertices"].size)


# ------------------------------------------------------------------ 3. bit identities
@pytest.mark.parametrize("name", ["chain17", "chain33", "chain65", "tets_strain"])
def test_pinned_paths_are_bit_identical(name):
    import torch
    frames, kinds, m, dt = _mesh(name)
    N = frames.shape[1]
    snaps = _snaps(frames)
    v = np.array([0, N // 2, N - 1])
    moving = dict(vertices=v, wi=np.array([0.7, 1e3, 2.0]), shift=pins.shift_of(3, 140), shift_start=1)
    for F in FRAMES:
        kw = dict(gravity=G, frame_end=F)
        for mode in MODES:
            # K = 1 from the frame is global_step: the constant is formed in the same order
            step = snaps.global_step(kinds, dt, m, velocity=mode, pins=moving, **kw)[0]
            assert torch.equal(snaps.solve_frames(kinds, dt, 1, m, velocity=mode, start="frame", pins=moving, **kw)[0], step)
            assert not torch.equal(snaps.global_step(kinds, dt, m, velocity=mode, **kw)[0], step)
            # one step of a roll-out is solve_frames from the explicit state
            q, q_prev, nF = snaps.simulate_frames(kinds, dt, 1, 3, m, velocity=mode, pins=moving, **kw)
            assert nF == F and torch.equal(q, snaps.solve_frames(kinds, dt, 3, m, velocity=mode, start="explicit", pins=moving, **kw)[0])
        want = snaps.simulate_frames(kinds, dt, 3, 2, m, record_every=1, pins=moving, **kw)
        # T1 steps continued by T2 with shift_start raised by T1 are T1 + T2 steps
        for a, b in ((1, 2), (2, 1)):
            q1, p1, _ = snaps.simulate_frames(kinds, dt, a, 2, m, pins=moving, **kw)
            later = dict(moving, shift_start=moving["shift_start"] + a)
            q2, p2, _ = snaps.simulate_frames(kinds, dt, b, 2, m, state=(q1, p1), pins=later, **kw)
            assert torch.equal(q2, want[0]) and torch.equal(p2, want[1]) and torch.equal(q1, want[3][0][a - 1])
            if F > 1:                                               # (not raised: another row, another result)
                assert not torch.equal(snaps.simulate_frames(kinds, dt, b, 2, m, state=(q1, p1), pins=moving, **kw)[0], want[0])
        # repeats, a chunk width and a frame sub-range (the rows follow the frames) change no bit
        assert torch.equal(snaps.simulate_frames(kinds, dt, 3, 2, m, record_every=1, pins=moving, **kw)[3][0], want[3][0])
        assert torch.equal(snaps.simulate_frames(kinds, dt, 3, 2, m, record_every=1, chunk_frames=16, pins=moving, **kw)[3][0], want[3][0])
        if F > 3:
            part = snaps.simulate_frames(kinds, dt, 3, 2, m, gravity=G, frame_start=1, frame_end=F, frame_jump=2, record_every=1, pins=moving)
            assert part[2] == len(range(1, F, 2)) and torch.equal(part[3][0], want[3][0][:, 1:F:2]) and torch.equal(part[1], want[1][1:F:2])
        # a shift of zeros is no shift; positions None are the rest positions a kind would take
        fixed = dict(vertices=v, wi=moving["wi"])
        zeros = dict(fixed, shift=np.zeros((140, 3, 3)))
        rest = dict(fixed, positions=frames[0][v])
        a = snaps.simulate_frames(kinds, dt, 2, 2, m, pins=fixed, **kw)
        assert torch.equal(snaps.simulate_frames(kinds, dt, 2, 2, m, pins=zeros, **kw)[0], a[0])
        assert torch.equal(snaps.simulate_frames(kinds, dt, 2, 2, m, pins=rest, **kw)[0], a[0])
        assert torch.equal(snaps.simulate_frames(kinds, dt, 2, 2, m, pins=dict(zeros, shift=np.zeros((140, 3))), **kw)[0], a[0])
        assert not torch.equal(a[0], want[3][0][1])


def test_a_pinned_run_after_one_of_another_shape_or_other_pins_equals_a_fresh_context_and_the_padding_stays_zero():
    import torch
    frames, kinds, m, dt = _mesh("chain33")
    N = frames.shape[1]
    P = dict(vertices=np.array([0, N - 1]), wi=np.array([1e3, 0.7]), shift=pins.shift_of(2, 80), shift_start=3)
    fresh = _snaps(frames[:65]).simulate_frames(kinds, dt, 3, 2, m, gravity=G, pins=P)
    big_frames, big_kinds, big_m, big_dt = _mesh("stiff")
    big = _snaps(big_frames[:5])
    big.simulate_frames(big_kinds, big_dt, 2, 2, big_m, pins=dict(vertices=np.arange(big_frames.shape[1]), wi=5.0))
    from animsnapbases_amd import posSnapshots
    with contextlib.redirect_stdout(io.StringIO()):
        small = posSnapshots.from_arrays(np.array(frames), None, "first", standarize=False, massWeight=False, engine=big._engine)
    # other pins on the same mesh, every column of the buffers filled with huge values, then fewer frames
    huge = torch.full((130, N, 3), 1e30, dtype=torch.float64, device=fresh[0].device)
    small.simulate_frames(kinds, dt, 2, 1, m, state=(huge, huge.clone()), pins=dict(vertices=np.arange(N), wi=1e3, shift=np.ones((140, 3))))
    got = small.simulate_frames(kinds, dt, 3, 2, m, gravity=G, frame_end=65, pins=P)
    assert torch.equal(got[0], fresh[0]) and torch.equal(got[1], fresh[1])
    for which in (0, 1):
        st = small._engine.pdsolve_state(which)
        assert st.shape == (3 * N, 128) and np.all(st[:, 65:] == 0.0) and np.isfinite(st[:, :65]).all()
    assert np.array_equal(small._engine.pdsolve_state(0)[:, :65].T.reshape(65, -1, 3), got[0].cpu().numpy())
    # and a run without pins afterwards is the run of a context that never saw any
    bare = _snaps(frames[:65]).simulate_frames(kinds, dt, 3, 2, m, gravity=G)
    after = small.simulate_frames(kinds, dt, 3, 2, m, gravity=G, frame_end=65)
    assert torch.equal(after[0], bare[0]) and torch.equal(after[1], bare[1]) and not torch.equal(after[0], got[0])


# ------------------------------------------------------------------ 4. refusals of the engine
def test_engine_refusals_return_their_code_and_launch_nothing():
    import torch
    from animsnapbases_amd import _lib
    frames, kinds, m, dt = _mesh("chain17")
    F, N = 5, frames.shape[1]
    snaps = _snaps(frames)
    eng = snaps._engine
    err = lambda: eng.lib.asb_last_error(eng.h)
    P = dict(vertices=np.array([0, N - 1]), wi=np.array([1.0, 2.0]))
    rec = snaps._pins("test", P)
    # before any solve
    eng.pins_set(rec.vertices, rec.wi, rec.p0, None)
    assert eng.lib.asb_pdsolve_pins(eng.h, 0) == _lib.ERR_ARG and b"no solve begun" in err()
    # what asb_pins_set refuses leaves no pins behind
    i64, f64 = lambda a: np.ascontiguousarray(a, dtype=np.int64), lambda a: np.ascontiguousarray(a, dtype=np.float64)
    ok_v, ok_w, ok_p = i64([0, 3]), f64([1.0, 2.0]), f64(np.zeros((2, 3)))
    bad = [(i64([0, N]), ok_w, ok_p, 0, None, b"names vertex"), (i64([-1, 2]), ok_w, ok_p, 0, None, b"names vertex"),
           (i64([3, 3]), ok_w, ok_p, 0, None, b"pinned twice"), (ok_v, f64([1.0, -1.0]), ok_p, 0, None, b"wi"),
           (ok_v, f64([np.nan, 1.0]), ok_p, 0, None, b"wi"), (ok_v, ok_w, f64(np.full((2, 3), np.inf)), 0, None, b"position"),
           (ok_v, ok_w, ok_p, 4, f64(np.full((4, 3), np.nan)), b"shift"), (ok_v, ok_w, ok_p, 4, None, b"rows of shift")]
    out = torch.zeros((F, N, 3), dtype=torch.float64, device="cuda:%d" % eng.device_id)
    for v, w, p, T_s, sh, msg in bad:
        assert eng.lib.asb_pins_set(eng.h, 2, _lib.ptr(v), _lib.ptr(w), _lib.ptr(p), T_s, _lib.ptr(sh), 0) == _lib.ERR_ARG and msg in err()
        assert eng.lib.asb_pins_term(eng.h, 0, F, 1, 0, 0, out.data_ptr()) == _lib.ERR_ARG and b"no pins" in err()
    assert eng.lib.asb_pins_set(eng.h, N + 1, _lib.ptr(i64(np.arange(N + 1))), _lib.ptr(f64(np.ones(N + 1))), _lib.ptr(f64(np.zeros((N + 1, 3)))),
                                0, None, 0) == _lib.ERR_ARG
    # a moving pin: rows 0 .. 6; frames 0 .. 4 read rows 2 .. 6 with row0 = 2
    sh = f64(np.zeros((7, 3)))
    eng.pins_set(rec.vertices, rec.wi, rec.p0, sh)
    assert eng.lib.asb_pins_term(eng.h, 0, F, 1, 3, 0, out.data_ptr()) == _lib.ERR_ARG and b"row 7 of the shift" in err()
    assert eng.lib.asb_pins_term(eng.h, 0, F, 1, -1, 0, out.data_ptr()) == _lib.ERR_ARG
    assert eng.lib.asb_pins_term(eng.h, 0, 0, 1, 0, 0, out.data_ptr()) == _lib.ERR_ARG and b"empty frame range" in err()
    good = snaps.simulate_frames(kinds, dt, 3, 2, m, frame_end=F, pins=dict(P, shift=sh))      # rows 0 .. 6: just enough
    eng.pins_set(rec.vertices, rec.wi, rec.p0, sh)
    eng.pdsolve_begin(0, 0, F, 1, None, False, 1.0, m / dt ** 2, 1, np.zeros(3), 0)
    assert eng.lib.asb_pdsolve_pins(eng.h, 3) == _lib.ERR_ARG and b"row 7 of the shift" in err()
    eng.pdsolve_pins(2)
    assert eng.lib.asb_pdsolve_pins(eng.h, 2) == _lib.ERR_ARG and b"already" in err()           # (the term would be added twice)
    eng.pdsolve_carry(None)
    before = eng.pdsolve_state(0)
    assert eng.lib.asb_pdsolve_advance(eng.h) == _lib.ERR_ARG and b"row 7 of the shift" in err()
    assert np.array_equal(eng.pdsolve_state(0), before) and np.array_equal(eng.pdsolve_state(1)[:, :F].T.reshape(F, N, 3), frames[:F])
    # a begin drops the binding: the advance is the plain one again; clearing the pins drops it too
    eng.pdsolve_begin(0, 0, F, 1, None, False, 1.0, m / dt ** 2, 1, np.zeros(3), 0)
    eng.pdsolve_carry(None)
    eng.pdsolve_advance()
    eng.pdsolve_pins(1)
    eng.pins_clear()
    eng.pdsolve_advance()
    assert eng.lib.asb_pdsolve_pins(eng.h, 0) == _lib.ERR_ARG and b"no pins" in err()
    # pins checked against another tensor are refused
    eng.pins_set(rec.vertices, rec.wi, rec.p0, None)
    from animsnapbases_amd import posSnapshots
    with contextlib.redirect_stdout(io.StringIO()):
        wide = posSnapshots.from_arrays(np.array(_mesh("chain33")[0]), None, "first", standarize=False, massWeight=False, engine=eng)
    wide_out = torch.zeros((F, 33, 3), dtype=torch.float64, device=out.device)
    assert eng.lib.asb_pins_term(eng.h, 0, F, 1, 0, 0, wide_out.data_ptr()) == _lib.ERR_ARG and b"checked against" in err()
    del wide
    torch.cuda.synchronize()
    assert torch.equal(out, torch.zeros_like(out)) and torch.equal(wide_out, torch.zeros_like(wide_out))      # no refused call wrote anything
    # the public layer refuses a vertex >= N before the engine, and the object still works
    with pytest.raises(ValueError, match="outside"):
        snaps.simulate_frames(kinds, dt, 3, 2, m, frame_end=F, pins=dict(P, vertices=[0, N]))
    snaps = _snaps(frames)
    again = snaps.simulate_frames(kinds, dt, 3, 2, m, frame_end=F, pins=dict(P, shift=sh))
    assert torch.equal(again[0], good[0]) and torch.equal(again[1], good[1])
