"""GPU (-m gpu): time steps on a resident animation -- asb_pdsolve_carry / _advance / _positions of csrc/asb_pdsolve.hip and
posSnapshots.simulate_frames / reduced_rollout_errors -- against the fixtures of the UNMODIFIED reference's own code
(tools/gen_golden_rollout.py: ``reference_loop`` per step, Simulators.py:531-532 between steps; start frames range(0, 130, 3),
K in {1, 3, 10}, T in rollout_cases.STEPS), against the host route of tests/rollout_cases.py for the reduced kind, step by
step against one NumPy iteration from the device's OWN two previous records (no amplification enters), and bit for bit
against ``solve_frames`` and against itself.

Shapes.  k_pd_advance's tile is 64 rows (3 v + d) x 64 frames: chains of N in {2, 15, 16, 17, 21, 22, 31, 32, 33, 65} vertices
(3 N = 63 and 66 straddle the row tile) at F' in {1, 63, 64, 65, 130}, and the goldens (N = 18, 42; F' = 44).

Bounds: B = 2 max(1, amp_T) T (K one + adv) of tests/rollout_cases.py, amp_T measured on the host model and stored with the
fixtures.  No start frame is left out of any comparison.  Every measured error is printed beside its bound."""
import contextlib
import io

import numpy as np
import pytest
from scipy import sparse
from scipy.sparse.linalg import splu

from conftest import load_golden
from gstep_cases import EPS, golden
from pdsolve_cases import host_case
from reduced_forces_cases import case as rf_case, operator as rf_operator
from rollout_cases import KS, MODES, NAMES, REDUCED, START_FRAMES, STEPS, adv_bound, bound_T, iterate, rollout, start_state
from test_gpu_cforces import _bound as force_bound, _g
from test_gpu_cproj import _kappa, _min_edge
from test_gpu_gstep import _case, _report
from test_gpu_pdsolve import _mesh, _reduced_kw, _reduced_one, _snaps

pytestmark = pytest.mark.gpu

CHAINS = [2, 15, 16, 17, 21, 22, 31, 32, 33, 65]
FRAMES = [1, 63, 64, 65, 130]
SEL = dict(frame_jump=3)                                            # range(0, 130, 3): START_FRAMES
G = (0.0, -9.81, 0.3)


def _dev(snaps, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:%d" % snaps._engine.device_id)


def _prev(frames, sel):
    return frames[[max(f - 1, 0) for f in sel]]


# ------------------------------------------------------------------ 1. against the reference's time steps
def _against_reference(name, snaps, z, kinds, one, tag):
    p = load_golden("rollout_" + name)
    worst, b_lo, b_hi = 0.0, np.inf, 0.0
    T = max(STEPS[name])
    for mode in MODES:
        for K in KS:
            q, q_prev, nF, (rec, steps) = snaps.simulate_frames(kinds, float(z["dt"]), T, K, z["masses"], velocity=mode, record_every=1, **SEL)
            assert nF == len(START_FRAMES) and steps == list(range(1, T + 1)) and tuple(rec.shape[:2]) == (T, nF)
            got = rec.cpu().numpy()
            assert np.array_equal(q.cpu().numpy(), got[-1]) and np.array_equal(q_prev.cpu().numpy(), got[-2])
            for t in STEPS[name]:
                ref = p["q_%s_%d_%d" % (mode, K, t)]
                B = bound_T(one[mode], K, t, float(p["amp_%s_%d_%d" % (mode, K, t)]), adv_bound(ref, ref))
                err = _report("%s %s K = %d T = %d %s" % (name, mode, K, t, tag), got[t - 1], ref, B)
                assert err <= B
                assert np.abs(got[t - 1] - got[0]).max() > B        # the steps move: not the one-step result
                worst, b_lo, b_hi = max(worst, err / B), min(b_lo, B), max(b_hi, B)
    print("%s %s: largest err / B %.3g, B in [%.3g, %.3g]" % (name, tag, worst, b_lo, b_hi))


@pytest.mark.parametrize("name", NAMES)
def test_rollout_matches_the_reference(name):
    z, frames, kinds, one = _case(name)
    _against_reference(name, _snaps(frames), z, kinds, one, "raw")


@pytest.mark.parametrize("name", NAMES)
def test_rollout_on_a_weighted_standardised_tensor(name):
    kind = "tets_strain" if name == "combined" else name
    g = _g(kind)[0]
    if name == "combined":
        tol_p = 64 * EPS * np.abs(g["frames"]).max() * max(_kappa(k, _g(k)[0]) / _min_edge(k, _g(k)[0]) for k in ("edge_spring", "tets_strain"))
    else:
        tol_p = 64 * EPS * np.abs(g["frames"]).max() / _min_edge(kind, g) * _kappa(kind, g)
    z, frames, kinds, one = _case(name, tol_p)
    mass = 0.5 + np.random.default_rng(3).random(frames.shape[1])   # the weighting of the tensor is not the solver's mass
    snaps = _snaps(frames, standarize=True, mass=mass)
    assert snaps.pre_scale_factor != 1 and snaps.massL is not None
    _against_reference(name, snaps, z, kinds, one, "weighted")


# (a reduced fixture whose amp_T leaves the cap at T = 2 already keeps no step -- tets_deim -- and is covered by sections 2 and 3)
@pytest.mark.parametrize("fixture", [f for f in sorted(REDUCED) if load_golden("rollout_reduced_" + f)["steps"].size])
def test_reduced_rollout_matches_the_host_route(fixture):
    c = rf_case(fixture)
    z = golden(c.kind)
    hc = host_case(c.kind)
    amps = load_golden("rollout_reduced_" + fixture)
    steps = amps["steps"].tolist()
    frames = c.g["frames"]
    dt, masses = float(z["dt"]), z["masses"]
    snaps = _snaps(frames)
    T = max(steps)
    for m in (c.ms[0], c.ms[-1]):
        op = rf_operator(c, m)
        spec = dict(kind=c.kind, basis=c.basis, num_components=m, reduction=c.reduction, **_reduced_kw(c))
        for mode in MODES:
            s, x = start_state(frames, START_FRAMES, mode)
            for K in KS:
                host = rollout(hc, K, T, s, x, reduced=(0, op))
                rec = snaps.simulate_frames([spec], dt, T, K, masses, velocity=mode, record_every=1, **SEL)[3][0].cpu().numpy()
                hy = snaps.simulate_frames([spec], dt, T, K, masses, velocity=mode, record_every=1, hyper="touched", **SEL)[3][0].cpu().numpy()
                for t in steps:
                    B = bound_T(_reduced_one(c, z, m, host[t - 1]), K, t, float(amps["amp_%d_%s_%d_%d" % (m, mode, K, t)]),
                                adv_bound(host[t - 1], host[t - 1]))
                    assert _report("%s m = %d %s K = %d T = %d" % (fixture, m, mode, K, t), rec[t - 1], host[t - 1], B) <= B
                    assert _report("%s m = %d %s K = %d T = %d hyper" % (fixture, m, mode, K, t), hy[t - 1], host[t - 1], B) <= B
                    assert np.abs(rec[t - 1] - rec[0]).max() > B


# ------------------------------------------------------------------ 2. every step against one host iteration of the device's own records
_chains = {}


def _chain_case(n):
    """The chain of n vertices as a case of ``pdsolve_cases.host_case`` with what the one-iteration bound needs."""
    if n not in _chains:
        from animsnapbases_amd import projections as proj
        frames, kinds, m, dt = _mesh("chain%d" % n)
        rest, edges = kinds[0]["rest_positions"], kinds[0]["elements"]
        setup = proj.build_setup("edge_spring", edges, rest)
        St = proj.assembly_ST(setup, n, kinds[0]["wi"])
        A = proj.global_matrix([(setup, kinds[0]["wi"])], n, m, dt)
        Ad = A.toarray()
        _chains[n] = dict(frames=frames, kinds=[(setup, St, 1.0, 1.0)], masses=m, dt=dt, lu=splu(sparse.csc_matrix(A)), spec=kinds,
                          Ainv_abs_inf=np.abs(np.linalg.inv(Ad)).sum(axis=1).max(), kappa=np.linalg.cond(Ad),
                          d=np.linalg.norm(rest[edges[:, 1]] - rest[edges[:, 0]], axis=1), edges=edges)
    return _chains[n]


def _chain_bound(c, s, q):
    """The one-iteration bound of gstep_cases for the iteration s -> q of a chain, plus the carry's rounding passed through
    A^-1 M / dt^2: || |A^-1| ||_inf max(diag) adv."""
    from animsnapbases_amd import projections as proj
    setup, St = c["kinds"][0][:2]
    ln = np.linalg.norm(s[:, c["edges"][:, 1]] - s[:, c["edges"][:, 0]], axis=2)
    tol_p = 64 * EPS * np.abs(s).max() / ln.min() * max(1.0, (c["d"][None] / ln).max())
    fb = force_bound(St, proj.project_host(setup, s, 1.0, 1.0), tol_p).max()
    one = c["Ainv_abs_inf"] * fb + 64 * EPS * c["kappa"] * np.abs(q).max()
    adv = 2.0 * EPS * (3.0 * np.abs(s).max() + np.abs(G).max())
    return one + c["Ainv_abs_inf"] * (c["masses"] / c["dt"] ** 2).max() * adv


@pytest.mark.parametrize("n", CHAINS)
def test_every_step_is_one_host_iteration_from_the_devices_own_records(n):
    c = _chain_case(n)
    frames, dt = c["frames"], c["dt"]
    acc = dt * dt * np.array(G)
    snaps = _snaps(frames)
    T = 4
    for F in FRAMES:
        for mode in MODES:
            q, q_prev, nF, (rec, steps) = snaps.simulate_frames(c["spec"], dt, T, 1, c["masses"], velocity=mode, gravity=G, record_every=1,
                                                                frame_end=F)
            assert nF == F and steps == [1, 2, 3, 4]
            r = rec.cpu().numpy()
            assert np.isfinite(r).all()
            x = frames[:F]
            hist = [x if mode == "zero" else _prev(frames, range(F)), x] + list(r)          # p_0 (so that 2 x - p_0 = s_1), x, q_1 ..
            worst = 0.0
            for t in range(1, T + 1):
                s = 2.0 * hist[t] - hist[t - 1] + acc[None, None, :]
                want = iterate(c, s, s, 1)
                B = _chain_bound(c, s, want)
                err = np.abs(r[t - 1] - want).max()
                worst = max(worst, err / B)
                assert err <= B, (n, F, mode, t, err, B)
            assert np.abs(r[3] - r[0]).max() > B                     # the steps move
            print("chain %d F' = %d %s: largest err / bound %.3g (bound %.3g)" % (n, F, mode, worst, B))


# ------------------------------------------------------------------ 3. bit identities
@pytest.mark.parametrize("name", ["chain17", "chain22", "chain65", "tris_strain"])
def test_first_step_state_and_continuation_are_bit_identical(name):
    import torch
    frames, kinds, m, dt = _mesh(name)
    snaps = _snaps(frames)
    X = _dev(snaps, frames)
    for F in FRAMES:
        kw = dict(gravity=G, frame_end=F)
        for mode in MODES:
            # (a) one step is solve_frames from the explicit state; q_prev is x_f
            q, q_prev, nF = snaps.simulate_frames(kinds, dt, 1, 3, m, velocity=mode, **kw)
            assert nF == F and torch.equal(q, snaps.solve_frames(kinds, dt, 3, m, velocity=mode, start="explicit", **kw)[0])
            assert torch.equal(q_prev, X[:F])
        # (b) the animation's own pair as a state is the start with velocity "difference": k_pd_advance's arithmetic is
        # k_gs_inertia's and k_pd_init's
        prev = _dev(snaps, _prev(frames, range(F)))
        want = snaps.simulate_frames(kinds, dt, 3, 2, m, velocity="difference", record_every=1, **kw)
        got = snaps.simulate_frames(kinds, dt, 3, 2, m, velocity="zero", state=(X[:F].clone(), prev), record_every=1, **kw)
        assert torch.equal(got[3][0], want[3][0]) and torch.equal(got[1], want[1]) and got[3][1] == want[3][1]
        # (c) T1 steps continued by T2 are T1 + T2 steps; (f) the records are the q of the shorter roll-outs
        for a, b in ((1, 2), (2, 1)):
            q1, p1, _ = snaps.simulate_frames(kinds, dt, a, 2, m, **kw)
            keep = (q1.clone(), p1.clone())
            q2, p2, _ = snaps.simulate_frames(kinds, dt, b, 2, m, state=(q1, p1), **kw)
            assert torch.equal(q2, want[0]) and torch.equal(p2, want[1])
            assert torch.equal(q1, want[3][0][a - 1]) and torch.equal(q1, keep[0]) and torch.equal(p1, keep[1])
        # a record every second step, the last step not recorded
        q, p, _, (rec, steps) = snaps.simulate_frames(kinds, dt, 3, 2, m, record_every=2, **kw)
        assert steps == [2] and torch.equal(rec[0], want[3][0][1]) and torch.equal(q, want[0]) and torch.equal(p, want[1])


@pytest.mark.parametrize("fixture", sorted(REDUCED))
def test_reduced_and_hyper_paths_continue_bit_identically(fixture):
    import torch
    c = rf_case(fixture)
    z = golden(c.kind)
    frames = c.g["frames"]
    dt, masses = float(z["dt"]), z["masses"]
    snaps = _snaps(frames)
    spec = [dict(kind=c.kind, basis=c.basis, num_components=c.ms[-1], reduction=c.reduction, **_reduced_kw(c))]
    whole = {}
    for hyper in (None, "touched", "all"):
        kw = dict(gravity=G, hyper=hyper)
        whole[hyper] = snaps.simulate_frames(spec, dt, 4, 3, masses, record_every=1, **kw)
        q1, p1, _ = snaps.simulate_frames(spec, dt, 3, 3, masses, **kw)
        q2, p2, _ = snaps.simulate_frames(spec, dt, 1, 3, masses, state=(q1, p1), **kw)
        assert torch.equal(q2, whole[hyper][0]) and torch.equal(p2, whole[hyper][1]) and torch.equal(p2, q1)
        # (e) repeats, a sub-range and a chunk width change no bit
        assert torch.equal(snaps.simulate_frames(spec, dt, 4, 3, masses, **kw)[0], whole[hyper][0])
        part = snaps.simulate_frames(spec, dt, 4, 3, masses, frame_start=3, frame_end=67, frame_jump=2, record_every=1, **kw)
        assert part[2] == 32 and torch.equal(part[3][0], whole[hyper][3][0][:, 3:67:2]) and torch.equal(part[1], whole[hyper][1][3:67:2])
        assert torch.equal(snaps.simulate_frames(spec, dt, 4, 3, masses, chunk_frames=16, record_every=1, **kw)[3][0], whole[hyper][3][0])
    # (d) "touched" is "all"
    assert torch.equal(whole["touched"][3][0], whole["all"][3][0]) and torch.equal(whole["touched"][1], whole["all"][1])
    assert not torch.equal(whole["all"][3][0][3], whole["all"][3][0][0])


@pytest.mark.parametrize("name", ["tets_strain", "combined"])
def test_repeats_ranges_and_chunks_are_bit_identical(name):
    import torch
    z, frames, kinds, _ = _case(name)
    dt, m = float(z["dt"]), z["masses"]
    snaps = _snaps(frames)
    for mode in MODES:
        kw = dict(velocity=mode, gravity=G, record_every=1)
        full = snaps.simulate_frames(kinds, dt, 3, 2, m, **kw)
        again = snaps.simulate_frames(kinds, dt, 3, 2, m, **kw)
        assert torch.equal(again[3][0], full[3][0]) and torch.equal(again[1], full[1])
        part = snaps.simulate_frames(kinds, dt, 3, 2, m, frame_start=3, frame_end=67, frame_jump=2, **kw)
        assert part[2] == 32 and torch.equal(part[3][0], full[3][0][:, 3:67:2]) and torch.equal(part[1], full[1][3:67:2])
        assert torch.equal(snaps.simulate_frames(kinds, dt, 3, 2, m, chunk_frames=16, **kw)[3][0], full[3][0])


def test_a_rollout_after_one_of_another_shape_equals_a_fresh_context_and_the_padding_stays_zero():
    import torch
    frames, kinds, m, dt = _mesh("chain33")
    fresh = _snaps(frames[:65]).simulate_frames(kinds, dt, 3, 2, m, gravity=G)
    big_frames, big_kinds, big_m, big_dt = _mesh("stiff")
    big = _snaps(big_frames[:5])
    big.simulate_frames(big_kinds, big_dt, 2, 2, big_m)
    from animsnapbases_amd import posSnapshots
    with contextlib.redirect_stdout(io.StringIO()):
        small = posSnapshots.from_arrays(np.array(frames), None, "first", standarize=False, massWeight=False, engine=big._engine)
    # every column of the buffers filled with huge values first, then fewer frames: (g) and (h)
    huge = torch.full((130, frames.shape[1], 3), 1e30, dtype=torch.float64, device=fresh[0].device)
    small.simulate_frames(kinds, dt, 2, 1, m, state=(huge, huge.clone()))
    got = small.simulate_frames(kinds, dt, 3, 2, m, gravity=G, frame_end=65)
    assert torch.equal(got[0], fresh[0]) and torch.equal(got[1], fresh[1])
    for which in (0, 1):
        st = small._engine.pdsolve_state(which)
        assert st.shape == (3 * frames.shape[1], 128) and np.all(st[:, 65:] == 0.0) and np.isfinite(st[:, :65]).all()
    # the state the hook shows is the result: Q the last positions, P the ones before
    assert np.array_equal(small._engine.pdsolve_state(0)[:, :65].T.reshape(65, -1, 3), got[0].cpu().numpy())
    assert np.array_equal(small._engine.pdsolve_state(1)[:, :65].T.reshape(65, -1, 3), got[1].cpu().numpy())


# ------------------------------------------------------------------ 4. NaN containment
def test_a_nan_frame_of_the_state_stays_in_its_frame():
    frames, kinds, m, dt = _mesh("chain33")
    snaps = _snaps(frames)
    for F, bad in ((65, 64), (130, 63)):
        for poisoned in (0, 1):
            state = [_dev(snaps, frames[:F]), _dev(snaps, _prev(frames, range(F)))]
            state[poisoned][bad, 5, 1] = float("nan")
            q, p, _, (rec, _) = snaps.simulate_frames(kinds, dt, 4, 2, m, state=tuple(state), record_every=1, gravity=G, frame_end=F)
            r = rec.cpu().numpy()
            nan = np.isnan(r).any(axis=(2, 3))
            assert nan[:, bad].all() and not np.delete(nan, bad, axis=1).any(), (F, poisoned)
            assert np.isnan(r[-1, bad]).all()                       # the solve spreads it over the frame's vertices


# ------------------------------------------------------------------ 5. reduced_rollout_errors
def test_reduced_rollout_errors():
    c = rf_case("tris_blocks")
    z = golden(c.kind)
    dt, masses = float(z["dt"]), z["masses"]
    kw = dict(reduction=c.reduction, frame_jump=3, **_reduced_kw(c))
    snaps = _snaps(c.g["frames"])
    rs = [1, c.ms[0], c.ms[-1]]
    got = snaps.reduced_rollout_errors(c.kind, c.basis, rs, dt, 4, 3, masses, record_every=2, **kw)
    assert got[5] == [2, 4] and all(a.shape == (len(rs), 2) and np.isfinite(a).all() for a in got[:5])
    # a sweep equals single calls
    for i, r in enumerate(rs):
        single = snaps.reduced_rollout_errors(c.kind, c.basis, [r], dt, 4, 3, masses, record_every=2, **kw)
        assert all(np.array_equal(single[j][0], got[j][i]) for j in range(5))
    # hyper="touched" gives the numbers of "all"
    t = snaps.reduced_rollout_errors(c.kind, c.basis, rs, dt, 4, 3, masses, record_every=2, hyper="touched", **kw)
    a = snaps.reduced_rollout_errors(c.kind, c.basis, rs, dt, 4, 3, masses, record_every=2, hyper="all", **kw)
    assert all(np.array_equal(t[j], a[j]) for j in range(5)) and t[5] == a[5]
    # more components: a smaller error at the last step
    print("tris_blocks fro at the last step: r = 1 %.3g, r = %d %.3g" % (got[0][0, -1], rs[-1], got[0][-1, -1]))
    assert got[0][-1, -1] < got[0][0, -1]
    # one step: the lists of reduced_solve_errors
    for hyper in (None, "touched"):
        one = snaps.reduced_rollout_errors(c.kind, c.basis, rs, dt, 1, 3, masses, record_every=1, hyper=hyper, **kw)
        old = snaps.reduced_solve_errors(c.kind, c.basis, rs, dt, 3, masses, hyper=hyper, **kw)
        assert one[5] == [1] and all(one[j][:, 0].tolist() == old[j] for j in range(5))
    empty = snaps.reduced_rollout_errors(c.kind, c.basis, [], dt, 4, 3, masses, record_every=2, **kw)
    assert empty[5] == [2, 4] and all(e.shape == (0, 2) for e in empty[:5])


# ------------------------------------------------------------------ 6. refusals of the engine
def test_engine_refusals():
    import torch
    from animsnapbases_amd import _lib
    frames, kinds, m, dt = _mesh("chain17")
    F, N = 5, frames.shape[1]
    snaps = _snaps(frames)
    eng = snaps._engine
    out = torch.zeros((F, N, 3), dtype=torch.float64, device="cuda:%d" % eng.device_id)
    # before any solve: each entry returns its code, nothing is launched
    assert eng.lib.asb_pdsolve_carry(eng.h, None) == _lib.ERR_ARG and b"no solve begun" in eng.lib.asb_last_error(eng.h)
    assert eng.lib.asb_pdsolve_advance(eng.h) == _lib.ERR_ARG and b"no solve begun" in eng.lib.asb_last_error(eng.h)
    with pytest.raises(RuntimeError, match="no solve begun"):
        eng.pdsolve_positions(out.data_ptr())
    good = snaps.simulate_frames(kinds, dt, 2, 2, m, frame_end=F)
    # a solve without a carry refuses the advance and the positions
    snaps.solve_frames(kinds, dt, 1, m, frame_end=F)
    with pytest.raises(RuntimeError, match="asb_pdsolve_carry"):
        eng.pdsolve_advance()
    with pytest.raises(RuntimeError, match="asb_pdsolve_carry"):
        eng.pdsolve_positions(out.data_ptr())
    eng.pdsolve_carry(None)
    eng.pdsolve_advance()
    # a begin in between clears the carry
    eng.pdsolve_begin(0, 0, F, 1, None, False, 1.0, m / dt ** 2, 1, np.zeros(3), 0)
    assert eng.lib.asb_pdsolve_advance(eng.h) == _lib.ERR_ARG and b"asb_pdsolve_carry" in eng.lib.asb_last_error(eng.h)
    assert eng.lib.asb_pdsolve_positions(eng.h, None) == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(out, torch.zeros_like(out))                   # no refused call wrote anything
    # a malformed state, at the public layer
    dev = out.device
    for bad in ((out, out[:4].contiguous()), (out, torch.zeros((F, N + 1, 3), dtype=torch.float64, device=dev)),
                (torch.zeros((F, 3, N), dtype=torch.float64, device=dev).transpose(1, 2), out), (out, out.cpu())):
        with pytest.raises(ValueError, match="state"):
            snaps.simulate_frames(kinds, dt, 2, 2, m, frame_end=F, state=bad)
    again = snaps.simulate_frames(kinds, dt, 2, 2, m, frame_end=F)
    assert torch.equal(again[0], good[0]) and torch.equal(again[1], good[1])      # and the object still works
