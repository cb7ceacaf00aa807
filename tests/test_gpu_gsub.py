"""GPU (-m gpu): the global step in a position subspace q = o + U z -- asb_gsub_setup and the two product kernels of
csrc/asb_gsub.hip, the dispatch of asb_gstep_run / asb_pdsolve_* / asb_hyper_* on what the context holds, and every public method of
``posSnapshots`` that applies the global step under ``set_global_solver("subspace")``.

1. The two products alone through asb_test_gsub_apply against the longdouble model of tests/gsub_model.py: edge-spring chains of
   N in {2, 15, 16, 17, 31, 32, 33, 65}, r in {1, 3, 4, 17, N} where N allows (rp = 4 and 20, tiles of Y with 1 and with more than
   32 rows, N no multiple of 4), w in {1, 63, 64, 65, 130} columns, the affine and the linear map.
2. The unmodified reference through the FULL basis (r = N, where the Galerkin step is A^-1) on the five gstep_* / pdsolve_*
   fixtures.
3. r in {4, 8} on the same fixtures against the host model: plain, reduced kinds, ``hyper``; roll-outs T in {2, 5} on all five
   fixtures and with both pin fixtures of tests/pins_cases.py; hyper-reduced roll-outs with ``record_every``.
4. Bit identity under "subspace" (torch.equal).
5. ``subspace_solve_errors``.
6. Refusals.
Bounds: tests/gsub_cases.py derives them; every measured error is printed beside its bound.  No frame, column or case is left out.

Largest err / bound measured on an MI355X: 1. 0.027; 2. 3.3e-3; 3. plain 9.1e-4, reduced kinds and ``hyper`` 5.8e-4, roll-outs (five
fixtures, both pin fixtures) 7.5e-4 (also in DESIGN.md 3.20).  Every test here fails on the parent commit, where "subspace" is a ValueError."""
import contextlib
import io

import numpy as np
import pytest
from scipy import sparse

from conftest import load_golden
from gslab_model import chain_matrix
from gstep_cases import golden
from gsub_cases import RANKS, amps, apply_bound, hyper_bound, p_abs_inf, residual_bound, rhs_of, setup_residual_bound, sub_case
from gsub_model import EPS, Galerkin, svd_basis, vertex_major
from pdsolve_cases import KS, MODES, NAMES, bound_K, explicit_state, host_case, model
from reduced_forces_cases import bound as rf_bound, case as rf_case, operator as rf_operator
from test_gpu_cforces import _bound as force_bound, _g
from test_gpu_cproj import RAW_TOL
from test_gpu_gstep import _case, _report
from test_gpu_hyper import _identities, _spec as hyper_spec
from test_gpu_pdsolve import _mesh
from test_gpu_rollout import SEL

pytestmark = pytest.mark.gpu

CHAINS = [2, 15, 16, 17, 31, 32, 33, 65]
RS = [1, 3, 4, 17]
WIDTHS = [1, 63, 64, 65, 130]


def _snaps(frames, basis=None, r=None, origin=None, engine=None):
    from animsnapbases_amd import posSnapshots
    kw = {} if engine is None else dict(engine=engine)
    with contextlib.redirect_stdout(io.StringIO()):
        s = posSnapshots.from_arrays(np.array(frames), None, "first", standarize=False, massWeight=False, **kw)
    if basis is not None:
        s.set_global_solver("subspace", basis=basis, num_components=r, origin=origin)
    return s


def _fixture_snaps(name_or_frames, r):
    """Snapshots of a fixture's frames under the fixtures' subspace of r components (None: all N)."""
    frames = host_case(name_or_frames)["frames"] if isinstance(name_or_frames, str) else name_or_frames
    return _snaps(frames, svd_basis(frames), r, frames[0])


# ------------------------------------------------------------------ 1. the two products alone
@pytest.mark.parametrize("n", CHAINS)
def test_products_on_chains(n):
    from animsnapbases_amd import projections as proj
    rng = np.random.default_rng(300 + n)
    A = chain_matrix(n)
    eng = _snaps(rng.standard_normal((2, n, 3)))._engine
    comps = rng.standard_normal((n, n, 3))
    origin = rng.standard_normal((n, 3))
    R = rng.standard_normal((3 * n, max(WIDTHS))) * 10.0 ** rng.integers(-2, 3, size=(3 * n, 1))
    worst = 0.0
    for r in sorted(set(k for k in RS + [n] if k <= n)):
        Qt = proj.subspace_basis(comps, r)
        resid = eng.gsub_setup(A, Qt, origin)
        info = eng.gsub_info().tolist()
        assert info == [r, (r + 15) // 16 * 16, (n + 31) // 32 * 32, (r + 3) // 4 * 4]
        g = Galerkin(A, Qt, origin)
        rb = setup_residual_bound(g)
        assert 0.0 <= resid <= rb, (n, r, resid, rb)
        W, Ai, op, Ut = eng.gsub_state()
        assert np.array_equal(Ut, Qt)
        for d in range(3):
            assert np.abs(Ai[d] - g.Ai[d]).max() <= 64 * EPS * g.kappa[d] * float(np.abs(g.Ai[d]).max())
        assert np.abs(op - g.op).max() <= apply_bound(g, np.zeros((3 * n, 1)), True)
        for affine in (True, False):
            wide = None
            for w in sorted(WIDTHS, reverse=True):
                got = eng.gsub_apply(R[:, :w], affine)
                assert got.shape[1] == (w + 63) // 64 * 64 and np.isnan(got[:, w:]).all()       # the padding is never written
                got = got[:, :w]
                assert np.isfinite(got).all()
                ref = g.apply(R[:, :w], affine)
                bnd = apply_bound(g, R[:, :w], affine, np.abs(ref).max())
                err = float(np.abs(got - ref).max())                                        # every entry
                worst = max(worst, err / bnd)
                assert err <= bnd, (n, r, w, affine, err, bnd)
                res, resb = g.residual(got, R[:, :w]), residual_bound(g, bnd)      # U^T (A q - rhs) = 0 for both maps (U^T A o' = 0)
                assert res <= resb, (n, r, w, affine, res, resb)
                if wide is None:
                    wide = got
                assert np.array_equal(got, wide[:, :w])             # a column does not depend on the columns around it
    print("chain %d: largest err / bound %.3g" % (n, worst))
    assert worst < 1.0


# ------------------------------------------------------------------ bounds of the public path
def _fb(name):
    """The largest force bound of a fixture's element set at its frames' projections (tests/test_gpu_gstep.py's)."""
    if name == "combined":
        c = load_golden("st_combined")
        return float((force_bound(_g("edge_spring")[2], c["p_edge"], RAW_TOL) + force_bound(_g("tets_strain")[2], _g("tets_strain")[0]["expected"], RAW_TOL)).max())
    g, _, St = _g(name)
    return float(force_bound(St, g["expected"], RAW_TOL).max())


def _own(s, q_prev, state, reduced=None, extra=None):
    """The subspace's own bound of the iteration that starts at ``q_prev`` (gsub_cases.apply_bound on that right-hand side)."""
    return apply_bound(s["galerkin"], vertex_major(rhs_of(s, q_prev, state, reduced, extra)), True)


# ------------------------------------------------------------------ 2. the unmodified reference through the full basis
@pytest.mark.parametrize("name", NAMES)
def test_the_full_basis_reproduces_the_reference(name):
    z, frames, kinds, bnd = _case(name)
    p = load_golden("pdsolve_" + name)
    s = sub_case(name, None)
    F, N = frames.shape[:2]
    dt, m = float(z["dt"]), z["masses"]
    snaps, inv = _fixture_snaps(np.array(frames), None), _snaps(frames)
    worst = 0.0
    for mode in MODES:
        state = explicit_state(s["frames"], range(F), mode)
        B = bnd[mode] + _own(s, np.array(s["frames"]), state)
        out, nF = snaps.global_step(kinds, dt, m, velocity=mode)
        assert nF == F and tuple(out.shape) == (F, N, 3) and out.is_cuda
        got = out.cpu().numpy()
        err = _report("%s %s global_step r = N" % (name, mode), got, z["q_" + mode], B)
        assert err <= B
        other = inv.global_step(kinds, dt, m, velocity=mode)[0].cpu().numpy()
        assert _report("%s %s global_step r = N against inverse" % (name, mode), got, other, B + bnd[mode]) <= B + bnd[mode]
        worst = max(worst, err / B)
        host = model(s, range(F), mode, tuple(range(11)))
        amp = amps(s, mode)
        for K in KS:
            a_fix = float(p["amp_%s_%d" % (mode, K)])
            B = bound_K(bnd[mode] + _own(s, host[K - 1], state), K, max(a_fix, amp[K]))
            got = snaps.solve_frames(kinds, dt, K, m, velocity=mode)[0].cpu().numpy()
            err = _report("%s %s K = %d r = N" % (name, mode, K), got, p["q_%s_%d" % (mode, K)], B)
            assert err <= B
            worst = max(worst, err / B)
            other = inv.solve_frames(kinds, dt, K, m, velocity=mode)[0].cpu().numpy()
            both = B + bound_K(bnd[mode], K, a_fix)
            assert _report("%s %s K = %d r = N against inverse" % (name, mode, K), got, other, both) <= both
    assert snaps.global_solve_subspace == N and snaps.global_solve_residual <= setup_residual_bound(s["galerkin"])
    assert abs(snaps.global_matrix.toarray() - z["A"]).max() <= 1e-13 * np.abs(z["A"]).max()
    print("%s r = N: largest err / bound %.3g" % (name, worst))


# ------------------------------------------------------------------ 3. r in {4, 8} against the host model
@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("name", NAMES)
def test_a_small_subspace_matches_the_host_model(name, r):
    z, frames, kinds, _ = _case(name)
    s = sub_case(name, r)
    g = s["galerkin"]
    F = frames.shape[0]
    dt, m = float(z["dt"]), z["masses"]
    snaps, inv = _fixture_snaps(np.array(frames), r), _snaps(frames)
    fb, pinf = _fb(name), p_abs_inf(g)
    worst = 0.0
    for mode in MODES:
        state = explicit_state(s["frames"], range(F), mode)
        host = model(s, range(F), mode, tuple(range(11)))
        amp = amps(s, mode)
        step = snaps.global_step(kinds, dt, m, velocity=mode)[0].cpu().numpy()
        B = pinf * fb + _own(s, np.array(s["frames"]), state)
        ref = model(s, range(F), mode, (1,), start="frame")[1]
        assert _report("%s r = %d %s global_step" % (name, r, mode), step, ref, B) <= B
        for K in KS:
            B = bound_K(pinf * fb + _own(s, host[K - 1], state), K, amp[K])
            got = snaps.solve_frames(kinds, dt, K, m, velocity=mode)[0].cpu().numpy()
            err = _report("%s r = %d %s K = %d" % (name, r, mode, K), got, host[K], B)
            assert err <= B
            worst = max(worst, err / B)
        # not vacuous: the full solve is somewhere else, by more than the bound
        full = inv.solve_frames(kinds, dt, 10, m, velocity=mode)[0].cpu().numpy()
        assert np.abs(full - got).max() > 100 * B
    assert snaps.global_solve_subspace == r
    print("%s r = %d: largest err / bound %.3g" % (name, r, worst))


def _hyper_parts(s, c, op, q, state):
    """ms (F', N, 3), M (3, N, mp) = S^T V_d and coef (3, mp, F') of the iteration that starts at q."""
    from animsnapbases_amd import projections as proj
    setup, St, smin, smax = s["kinds"][0]
    P = proj.project_host(setup, q, smin, smax)[:, op.Pt]
    M = np.stack([St @ op.V[:, :, d] for d in range(3)])
    coef = np.stack([op.H[d] @ P[:, :, d].T for d in range(3)])
    return (s["masses"] / s["dt"] ** 2)[None, :, None] * state, M, coef


@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("fixture", ["tets_deim", "tris_blocks"])
def test_reduced_kinds_and_hyper_in_a_small_subspace_match_the_host_model(fixture, r):
    from hyper_cases import reduced_force_bound
    c = rf_case(fixture)
    z = golden(c.kind)
    s = sub_case(c.kind, r)
    g = s["galerkin"]
    frames = c.g["frames"]
    F = frames.shape[0]
    dt, masses = float(z["dt"]), z["masses"]
    snaps = _fixture_snaps(np.array(frames), r)
    pinf, fb = p_abs_inf(g), _fb(c.kind)
    worst = 0.0
    for mi in (c.ms[0], c.ms[-1]):
        op = rf_operator(c, mi)
        red = (0, op)
        for mode in MODES:
            state = explicit_state(s["frames"], range(F), mode)
            host = model(s, range(F), mode, tuple(range(11)), reduced=red)
            amp = amps(s, mode, reduced=red)
            for K in KS:
                one = pinf * max(fb, float(rf_bound(c, mi, op).max())) + _own(s, host[K - 1], state, red)
                B = bound_K(one, K, amp[K])
                out = snaps.solve_frames([hyper_spec(c, mi)], dt, K, masses, velocity=mode)[0].cpu().numpy()
                err = _report("%s r = %d m = %d %s K = %d reduced" % (fixture, r, mi, mode, K), out, host[K], B)
                assert err <= B
                ms, M, coef = _hyper_parts(s, c, op, host[K - 1], state)
                redb = float(reduced_force_bound(c.St, op, c.p_pt(mi), c.r["cond_%d" % mi], RAW_TOL, c.St.shape[0]).max())
                Bh = bound_K(pinf * max(fb, redb) + hyper_bound(g, ms, M, coef, np.abs(host[K]).max()), K, amp[K])
                for hyper in ("touched", "all"):
                    out = snaps.solve_frames([hyper_spec(c, mi)], dt, K, masses, velocity=mode, hyper=hyper)[0].cpu().numpy()
                    e = _report("%s r = %d m = %d %s K = %d %s" % (fixture, r, mi, mode, K, hyper), out, host[K], Bh)
                    assert e <= Bh
                    worst = max(worst, e / Bh, err / B)
    # reduced_solve_errors: the numbers of single calls
    kw = dict(reduction=c.reduction, elements=c.g["elements"], wi=0.7, rest_positions=c.g["rest"], sigma_min=c.g["sigma"][0], sigma_max=c.g["sigma"][1])
    rs = [c.ms[0], c.ms[-1]]
    for hyper in (None, "touched"):
        sweep = snaps.reduced_solve_errors(c.kind, c.basis, rs, dt, 3, masses, hyper=hyper, **kw)
        for i, mi in enumerate(rs):
            single = snaps.reduced_solve_errors(c.kind, c.basis, [mi], dt, 3, masses, hyper=hyper, **kw)
            assert [v[0] for v in single] == [sweep[j][i] for j in range(5)] and np.isfinite([v[0] for v in single]).all()
    print("%s r = %d: largest err / bound %.3g" % (fixture, r, worst))


def _rollout_cases():
    import pins_cases as pins
    return [("free", n) for n in NAMES] + [("pins", n) for n in sorted(pins.FIXTURES)]


@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("what,name", _rollout_cases())
def test_rollouts_in_a_small_subspace_match_the_host_model(what, name, r):
    """``simulate_frames`` T in {2, 5} (the records of one roll-out of 5 steps, ``record_every=1``) on the five fixtures without
    pins and on both pin fixtures of tests/pins_cases.py (fixed pins on the edge springs; a moving per-pin shift on edges +
    tetrahedra).  amp: rollout_cases' / pins_cases' measurement on the host model under the subspace (at most 93 here)."""
    import pins_cases as pins
    import rollout_cases as rc
    from pdsolve_cases import parts_of
    from test_pins_cpu import kinds_force_bound
    pinned = what == "pins"
    base = pins.FIXTURES[name]["base"] if pinned else name
    z, frames, kinds, _ = _case(base)
    dt, masses = float(z["dt"]), z["masses"]
    P = pins.pins_of(name, load_golden("cproj_" + parts_of(base)[-1])["rest"]) if pinned else None
    s = sub_case(base, r, base=pins.host_case(name)) if pinned else sub_case(base, r)
    g = s["galerkin"]
    snaps = _fixture_snaps(np.array(frames), r)
    sel = rc.START_FRAMES
    fb = float(kinds_force_bound(name).max()) if pinned else _fb(base)
    # (the pinned model measures its amplification with gravity on, rollout_cases' without: each run takes its model's)
    acc = dt * dt * np.array(pins.G) if pinned else None
    kw = dict(gravity=pins.G, **SEL) if pinned else dict(SEL)
    worst, Tmax = 0.0, 5
    for mode in MODES:
        for K in (1, 3):
            s0, p0 = rc.start_state(s["frames"], sel, mode, acc)
            if pinned:
                amp = pins.measure_amp(s, mode, K, Tmax, sel, acc)
                host = pins.rollout(s, K, Tmax, s0, p0, sel, acc)
            else:
                amp = rc.measure_amp(s, mode, K, Tmax, sel)
                host = rc.rollout(s, K, Tmax, s0, p0)
            q, q_prev, nF, (rec, steps) = snaps.simulate_frames(kinds, dt, Tmax, K, masses, velocity=mode, pins=P, record_every=1, **kw)
            assert nF == len(sel) and steps == list(range(1, Tmax + 1))
            got = rec.cpu().numpy()
            assert np.array_equal(got[-1], q.cpu().numpy()) and np.array_equal(got[-2], q_prev.cpu().numpy())
            for T in (2, 5):
                rows = np.array(sel) + T - 1
                extra = pins.pin_term(s, rows) if pinned else None
                rounding = pins.pin_rounding(s, rows) if pinned else 0.0
                state = rc.carry(host[T - 2], p0 if T == 2 else host[T - 3], acc)[0]
                one = p_abs_inf(g) * (fb + rounding) + _own(s, host[T - 1], state, None, extra)
                B = rc.bound_T(one, K, T, float(amp[T - 1]), rc.adv_bound(host[T - 1], host[T - 1], acc))
                err = _report("%s %s r = %d %s K = %d T = %d" % (what, name, r, mode, K, T), got[T - 1], host[T - 1], B)
                assert err <= B
                worst = max(worst, err / B)
            if pinned and K == 3:           # without pins the roll-out is somewhere else, by more than the bound
                loose = snaps.simulate_frames(kinds, dt, Tmax, K, masses, velocity=mode, **kw)[0].cpu().numpy()
                assert np.abs(loose - got[-1]).max() > B
    print("roll-outs %s %s r = %d: largest err / bound %.3g" % (what, name, r, worst))


@pytest.mark.parametrize("fixture", ["tets_deim", "tris_blocks"])
def test_hyper_rollouts_in_a_subspace(fixture):
    """``simulate_frames(hyper=)`` under the subspace, the call the solver was built for: T = 2 steps of K = 3 against the host
    route (reduced kind, Galerkin step), "touched" = "all" = the bits of every record, continuation, sub-range, chunk width."""
    import torch
    import rollout_cases as rc
    from hyper_cases import reduced_force_bound
    c = rf_case(fixture)
    z = golden(c.kind)
    r, K, T = 8, 3, 2
    s = sub_case(c.kind, r)
    g = s["galerkin"]
    frames = np.array(c.g["frames"])
    dt, masses = float(z["dt"]), z["masses"]
    snaps = _fixture_snaps(frames, r)
    mi = c.ms[-1]
    op = rf_operator(c, mi)
    red, spec, sel = (0, op), [hyper_spec(c, mi)], rc.START_FRAMES
    pinf, fb = p_abs_inf(g), _fb(c.kind)
    redb = float(reduced_force_bound(c.St, op, c.p_pt(mi), c.r["cond_%d" % mi], RAW_TOL, c.St.shape[0]).max())
    for mode in MODES:
        s0, p0 = rc.start_state(s["frames"], sel, mode)
        host = rc.rollout(s, K, T, s0, p0, reduced=red)
        amp = rc.measure_amp(s, mode, K, T, sel, reduced=red)
        whole = {h: snaps.simulate_frames(spec, dt, T, K, masses, velocity=mode, record_every=1, hyper=h, **SEL) for h in (None, "touched", "all")}
        for t in (1, 2):
            state = s0 if t == 1 else rc.carry(host[0], p0)[0]
            ms, M, coef = _hyper_parts(s, c, op, host[t - 1], state)
            one = pinf * max(fb, redb, float(rf_bound(c, mi, op).max())) + hyper_bound(g, ms, M, coef, np.abs(host[t - 1]).max())
            B = rc.bound_T(one, K, t, float(amp[t - 1]), rc.adv_bound(host[t - 1], host[t - 1]))
            for h in (None, "touched"):
                got = whole[h][3][0][t - 1].cpu().numpy()
                assert _report("%s r = %d %s T = %d hyper %s" % (fixture, r, mode, t, h), got, host[t - 1], B) <= B
        assert torch.equal(whole["touched"][3][0], whole["all"][3][0]) and torch.equal(whole["touched"][1], whole["all"][1])
        kw = dict(velocity=mode, hyper="touched")
        q1, p1, _ = snaps.simulate_frames(spec, dt, 1, K, masses, **kw, **SEL)
        q2, p2, _ = snaps.simulate_frames(spec, dt, 1, K, masses, state=(q1, p1), hyper="touched", **SEL)
        assert torch.equal(q2, whole["touched"][0]) and torch.equal(p2, whole["touched"][1]) and torch.equal(p2, q1)
        assert torch.equal(snaps.simulate_frames(spec, dt, T, K, masses, chunk_frames=16, **kw, **SEL)[0], whole["touched"][0])
        part = snaps.simulate_frames(spec, dt, T, K, masses, frame_start=0, frame_end=67, frame_jump=6, **kw)
        assert part[2] == 12 and torch.equal(part[0], whole["touched"][0][:23:2])


# ------------------------------------------------------------------ 4. bit identity under "subspace"
@pytest.mark.parametrize("name", ["tets_strain", "tris_strain", "combined"])
def test_repeats_ranges_chunks_and_continuations_are_bit_identical(name):
    import torch
    z, frames, kinds, _ = _case(name)
    dt, m = float(z["dt"]), z["masses"]
    frames = np.array(frames)
    comps = svd_basis(frames)
    snaps = _fixture_snaps(frames, 8)
    for mode in MODES:
        full = snaps.solve_frames(kinds, dt, 3, m, velocity=mode)[0]
        assert torch.isfinite(full).all() and torch.equal(snaps.solve_frames(kinds, dt, 3, m, velocity=mode)[0], full)
        part, nF = snaps.solve_frames(kinds, dt, 3, m, velocity=mode, frame_start=3, frame_end=67, frame_jump=2)
        assert nF == 32 and torch.equal(part, full[3:67:2])
        assert torch.equal(snaps.solve_frames(kinds, dt, 3, m, velocity=mode, chunk_frames=16)[0], full)
        for k, l in ((1, 2), (2, 1)):
            first = snaps.solve_frames(kinds, dt, k, m, velocity=mode)[0]
            assert torch.equal(snaps.solve_frames(kinds, dt, l, m, velocity=mode, start=first)[0], full)
        step = snaps.global_step(kinds, dt, m, velocity=mode)[0]
        assert torch.equal(snaps.global_step(kinds, dt, m, velocity=mode, chunk_frames=16)[0], step)
        assert torch.equal(snaps.global_step(kinds, dt, m, velocity=mode, frame_start=3, frame_end=67, frame_jump=2)[0], step[3:67:2])
        assert torch.equal(snaps.solve_frames(kinds, dt, 1, m, velocity=mode, start="frame")[0], step)
        # global_solve on the caller's tensor: a frame does not depend on the frames around it
        rhs_dev = snaps.constraint_forces(kinds)[0]
        whole = snaps.global_solve(rhs_dev)
        for a, b in ((0, 1), (63, 65), (5, 70)):
            assert torch.equal(snaps.global_solve(rhs_dev[a:b].contiguous()), whole[a:b])
        # T1 + T2 time steps; one step is solve_frames(start="explicit")
        q3, p3, _ = snaps.simulate_frames(kinds, dt, 3, 2, m, velocity=mode, **SEL)
        q1, p1, _ = snaps.simulate_frames(kinds, dt, 1, 2, m, velocity=mode, **SEL)
        q2, p2, _ = snaps.simulate_frames(kinds, dt, 2, 2, m, state=(q1, p1), **SEL)
        assert torch.equal(q2, q3) and torch.equal(p2, p3)
        assert torch.equal(q1, snaps.solve_frames(kinds, dt, 2, m, velocity=mode, start="explicit", **SEL)[0])
    # "subspace" -> "inverse" -> back: each solver reproduces its own bits; the inverse's are those of a context that never
    # held a subspace
    want = snaps.solve_frames(kinds, dt, 3, m)[0]
    snaps.set_global_solver("inverse")
    inv = snaps.solve_frames(kinds, dt, 3, m)[0]
    assert torch.equal(inv, _snaps(frames).solve_frames(kinds, dt, 3, m)[0])
    snaps.set_global_solver("subspace", basis=comps, num_components=8, origin=frames[0])
    assert torch.equal(snaps.solve_frames(kinds, dt, 3, m)[0], want)
    assert float((inv - want).abs().max()) > 1e-3                           # (another step altogether, not rounding)


@pytest.mark.parametrize("fixture", ["tets_deim", "tris_blocks"])
def test_hyper_identities_in_a_subspace(fixture):
    c = rf_case(fixture)
    z = golden(c.kind)
    snaps = _fixture_snaps(np.array(c.g["frames"]), 8)
    _identities(snaps, hyper_spec(c, c.ms[-1]), float(z["dt"]), z["masses"], c.g["frames"].shape[0])     # "touched" = "all", repeats, ranges, chunks, K + L


def test_a_solve_after_one_of_another_shape_equals_a_fresh_context():
    import torch
    frames, kinds, m, dt = _mesh("chain33")
    frames = np.array(frames)
    fresh = _fixture_snaps(frames[:20], 4).solve_frames(kinds, dt, 3, m)[0]
    big_frames, big_kinds, big_m, big_dt = _mesh("stiff")
    big_frames = np.array(big_frames)
    big = _snaps(big_frames[:70], svd_basis(big_frames[:70], 17), None, big_frames[0])
    big.solve_frames(big_kinds, big_dt, 2, big_m)
    small = _snaps(frames[:20], svd_basis(frames[:20]), 4, frames[0], engine=big._engine)
    assert small._engine is big._engine
    assert torch.equal(small.solve_frames(kinds, dt, 3, m)[0], fresh)


# ------------------------------------------------------------------ 5. subspace_solve_errors
def test_subspace_solve_errors():
    name = "tets_strain"
    z, frames, kinds, bnd = _case(name)
    frames = np.array(frames)
    F, N = frames.shape[:2]
    dt, m, K = float(z["dt"]), z["masses"], 3
    comps = svd_basis(frames)
    snaps = _snaps(frames)
    rs = [4, 8, N]
    got = snaps.subspace_solve_errors(kinds, comps, rs, dt, K, m, per_frame=True, origin=frames[0])
    assert got[5].shape == (len(rs), F) and all(len(v) == len(rs) for v in got[:5])
    assert snaps._subspace_solver() is None and snaps._slab_solver() is None              # the selected solver is restored
    for i, r in enumerate(rs):                                                            # a sweep equals single calls
        single = snaps.subspace_solve_errors(kinds, comps, [r], dt, K, m, per_frame=True, origin=frames[0])
        assert [v[0] for v in single[:5]] == [got[j][i] for j in range(5)] and np.array_equal(single[5][0], got[5][i])
    # r = N: both tensors lie within their bounds of the exact iteration; r = 4: far above
    s = sub_case(name, None)
    state = explicit_state(s["frames"], range(F), "difference")
    host = model(s, range(F), "difference", tuple(range(K + 1)))
    amp = max(float(load_golden("pdsolve_" + name)["amp_difference_%d" % K]), amps(s, "difference")[K])
    B = bound_K(bnd["difference"] + _own(s, host[K - 1], state), K, amp) + bound_K(bnd["difference"], K, amp)
    print("subspace_solve_errors: max metric %.3g at r = N (bound %.3g), %.3g at r = 4" % (got[1][2] * np.abs(host[K]).max(), B, got[1][0] * np.abs(host[K]).max()))
    assert got[0][2] <= B * np.sqrt(3 * F * N)
    assert got[0][0] > 1e6 * B * np.sqrt(3 * F * N) and got[0][0] > got[0][1] > got[0][2]
    # under "slab" the full solve runs under the slab factor and the selection comes back
    snaps.set_global_solver("slab", 4)
    slab = snaps.subspace_solve_errors(kinds, comps, [4], dt, K, m, origin=frames[0])
    assert snaps._slab_solver() == 4 and abs(slab[0][0] - got[0][0]) <= 4 * B * np.sqrt(3 * F * N)
    assert snaps.subspace_solve_errors(kinds, comps, [], dt, K, m) == ([], [], [], [], [])


# ------------------------------------------------------------------ 6. refusals
def test_refusals_return_their_code_and_leave_no_solver():
    import torch
    from animsnapbases_amd import _lib, projections as proj
    n, r = 33, 5
    rng = np.random.default_rng(9)
    A = chain_matrix(n)
    eng = _snaps(rng.standard_normal((2, n, 3)))._engine
    Qt = proj.subspace_basis(rng.standard_normal((r, n, 3)))
    origin = rng.standard_normal((n, 3))
    good = torch.zeros((4, n, 3), dtype=torch.float64, device="cuda:%d" % eng.device_id)
    out = torch.empty_like(good)

    def no_solver():
        with pytest.raises(RuntimeError, match="asb_gstep_setup"):
            eng.gstep_run(good.data_ptr(), 4, out.data_ptr())
        assert eng.gsub_held(A, Qt, origin) is None
        with pytest.raises(RuntimeError, match="no position subspace"):
            eng.gsub_info()

    def held():
        eng.gsub_setup(A, Qt, origin)
        eng.gstep_run(good.data_ptr(), 4, out.data_ptr())
        assert torch.isfinite(out).all()

    # a basis with a zero row block: U^T A U is singular, the dense layer's error, no solver
    held()
    zero = Qt.copy()
    zero[1, 2] = 0.0
    with pytest.raises(RuntimeError) as e:
        eng.gsub_setup(A, zero, origin)
    assert "status -5" in str(e.value)                              # ASB_ERR_NUMERIC
    no_solver()
    # r > n, values that are not finite, the matrix checks of asb_gstep_setup under this entry's name
    held()
    a, p = np.ascontiguousarray(A.indptr, dtype=np.int64), _lib.ptr
    ai, ad = np.ascontiguousarray(A.indices, dtype=np.int64), np.ascontiguousarray(A.data)
    wide = np.zeros((3, n + 1, n))
    assert eng.lib.asb_gsub_setup(eng.h, n, p(a), p(ai), p(ad), n + 1, p(wide), p(origin), None) == _lib.ERR_ARG
    assert b"basis vectors" in eng.lib.asb_last_error(eng.h)
    eng._gsub = None
    no_solver()
    for bad_q, bad_o in ((np.where(np.arange(n) == 3, np.nan, Qt), origin), (Qt, np.where(np.arange(3) == 1, np.inf, origin))):
        held()
        with pytest.raises(RuntimeError, match="not finite"):
            eng.gsub_setup(A, np.ascontiguousarray(bad_q), np.ascontiguousarray(bad_o))
        no_solver()
    for broken, what in ((A[:-1, :-1].tocsr(), "rows"), (sparse.triu(A).tocsr(), "symmetric")):
        held()
        with pytest.raises(RuntimeError, match=what):
            eng.gsub_setup(broken, Qt[:, :, :broken.shape[0]].copy(), origin[:broken.shape[0]].copy())
        assert b"asb_gsub_setup" in eng.lib.asb_last_error(eng.h)
        no_solver()
    # counts before pointers: nothing behind them is read
    one = np.zeros(1, dtype=np.int64)
    assert eng.lib.asb_gsub_setup(eng.h, n, p(one), None, None, 0, p(origin), p(origin), None) == _lib.ERR_ARG
    assert eng.lib.asb_gsub_setup(eng.h, 0, p(one), None, None, 1, p(origin), p(origin), None) == _lib.ERR_ARG
    assert eng.lib.asb_gsub_setup(eng.h, n, p(one), None, None, 10 ** 6, p(origin), p(origin), None) == _lib.ERR_ARG
    # each set-up releases the other two; under the subspace the inverse's hook and the history are refused
    held()
    assert eng.lib.asb_test_gstep_inverse(eng.h, p(np.empty((n, n))), n) == _lib.ERR_ARG
    eng.gstep_setup(A)
    with pytest.raises(RuntimeError, match="no position subspace"):
        eng.gsub_info()
    eng.gslab_setup(A, proj.slab_plan(A, 4))
    eng.gsub_setup(A, Qt, origin)
    with pytest.raises(RuntimeError, match="no slab factor"):
        eng.gslab_info()
    frames, kinds, m, dt = _mesh("chain33")
    frames = np.array(frames)
    snaps = _fixture_snaps(frames[:5], 4)
    snaps.solve_frames(kinds, dt, 1, m)
    e2 = snaps._engine
    assert e2.lib.asb_pdsolve_iterate(e2.h, 1, 0, None, p(np.empty((1, 5, 2)))) == _lib.ERR_ARG
    assert b"history" in e2.lib.asb_last_error(e2.h)
    with pytest.raises(ValueError, match="history"):                # before the device is touched
        snaps.solve_frames(kinds, dt, 2, m, history=True)
