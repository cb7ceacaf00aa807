"""GPU (-m gpu): the global step's block-tridiagonal slab solver -- asb_gslab_setup and the sweep of csrc/asb_gslab.hip, the
dispatch of asb_gstep_run / asb_pdsolve_* / asb_hyper_* on what the context holds, and every public method of ``posSnapshots``
that applies A^-1 under ``set_global_solver("slab")``.

1. The sweep alone through asb_test_gslab_solve against the longdouble-refined host solution of tests/gslab_model.py: chains of
   N in {1, 2, 15, 16, 17, 31, 33, 65} at slab targets {1, 4, 16, one slab} (single-vertex slabs exercise the padding to 16) and
   w in {1, 63, 64, 65, 130} columns; the grids 6^3 (target 32), 10^3 with wi = 1e3 (kappa 57.5) and 8^3 with wi = 1e6 (kappa
   8.5e5, the residual held too).  Bound: 64 eps kappa(A) max |x|, nothing fitted.  Observed on the device, error / bound: see
   OBSERVED below; the host model stays within 0.1.
2. The public path under "slab" with a small slab_target (N = 18 and 42 give several slabs) against the fixtures of the
   UNMODIFIED reference (gstep_*, pdsolve_*, rollout_*) and the host model for ``hyper``, with the bounds of the existing tests;
   "slab" and "inverse" agree within the sum of their bounds.
3. Bit identity under "slab" (torch.equal).
4. The lifted limit: an edge-spring chain of 50 001 vertices (98 slabs at target 512).
5. Refusals at the C entry.
No frame and no column is left out of any comparison.  Every measured error is printed beside its bound."""
import contextlib
import io
import types

import numpy as np
import pytest
from scipy import sparse

from conftest import load_golden
from gslab_model import EPS, bound, chain_matrix, gershgorin_kappa, grid_matrix, refined_solve, rhs
from gstep_cases import KINDS, golden
from pdsolve_cases import KS, MODES, NAMES, animate, bound_K, chain, host_case, model
from reduced_forces_cases import case as rf_case, operator as rf_operator
from test_gpu_cforces import _bound as force_bound
from test_gpu_gstep import _case, _report
from test_gpu_hyper import _identities, _one as hyper_one, _spec as hyper_spec
from test_gpu_pdsolve import _mesh, _reduced_kw, _reduced_one
from rollout_cases import adv_bound, bound_T
from test_gpu_rollout import SEL, _against_reference

pytestmark = pytest.mark.gpu

# error / bound as measured on an MI355X (the largest of each group)
OBSERVED = {"chains": 1.4e-2, "grid 6^3": 8.1e-4, "grid 10^3": 1.7e-3, "stiff grid": 8.6e-4}
CHAINS = [1, 2, 15, 16, 17, 31, 33, 65]
WIDTHS = [1, 63, 64, 65, 130]
TARGET = 4                                      # the public tests: N = 18 -> 4+ slabs, N = 42 -> 6+


def _snaps(frames, slab=TARGET, engine=None, **kw):
    from animsnapbases_amd import posSnapshots
    if engine is not None:
        kw["engine"] = engine
    kw.setdefault("standarize", False)
    mass = kw.pop("mass", None)
    with contextlib.redirect_stdout(io.StringIO()):
        s = posSnapshots.from_arrays(np.array(frames), None, "first", massWeight=mass is not None, mass=mass, **kw)
    if slab is not None:
        s.set_global_solver("slab", slab)
    return s


def _engine(n):
    return _snaps(np.random.default_rng(n).standard_normal((2, n, 3)), slab=None)._engine


def _sweep(eng, A, target, B, ref, kappa, tag):
    """The factor of A at ``target`` and the sweep on every width; returns the largest error / bound."""
    from animsnapbases_amd import projections as proj
    n = A.shape[0]
    plan = proj.slab_plan(A, n if target is None else target)
    resid, (ns, sp) = eng.gslab_setup(A, plan)
    assert ns == len(plan.slab_ptr) - 1 and sp == (np.diff(plan.slab_ptr).max() + 15) // 16 * 16
    assert 0.0 <= resid <= 64 * EPS * kappa
    worst, wide = 0.0, None
    for w in sorted(WIDTHS, reverse=True):
        got = eng.gslab_solve(B[:, :w])
        assert np.isfinite(got).all()
        bnd = bound(kappa, ref[:, :w])
        err = float(np.abs(got.astype(np.longdouble) - ref[:, :w]).max())      # every column
        worst = max(worst, err / bnd)
        assert err <= bnd, (tag, target, w, err, bnd)
        if wide is None:
            wide = got
        assert np.array_equal(got, wide[:, :w])                                 # a column does not depend on the columns around it
    print("%s target %s: %d slabs (largest padded %d), kappa %.3g, resid %.3g, largest err / bound %.3g" % (tag, target, ns, sp, kappa, resid, worst))
    return worst


# ------------------------------------------------------------------ 1. the sweep alone
@pytest.mark.parametrize("n", CHAINS)
def test_sweep_on_chains(n):
    A = chain_matrix(n)
    eng = _engine(n)
    B = rhs(n, max(WIDTHS), 11 * n)
    ref = refined_solve(A, B)
    kappa = np.linalg.cond(A.toarray())
    worst = max(_sweep(eng, A, t, B, ref, kappa, "chain %d" % n) for t in (1, 4, 16, None))
    assert worst < 1.0


@pytest.mark.parametrize("nx,wi,m0,target", [(6, 1e3, 0.3, 32), (10, 1e3, 0.3, 256), (10, 1e3, 0.3, 64), (8, 1e6, 0.02, 64)])
def test_sweep_on_grids(nx, wi, m0, target):
    A = grid_matrix(nx, wi, m0)
    n = A.shape[0]
    eng = _engine(n)
    B = rhs(n, max(WIDTHS), 13 * nx)
    _sweep(eng, A, target, B, refined_solve(A, B), np.linalg.cond(A.toarray()), "grid %d^3 wi %g" % (nx, wi))


# ------------------------------------------------------------------ 2. the public path under "slab"
@pytest.mark.parametrize("name", KINDS + ["combined"])
def test_global_step_under_slab_matches_the_reference(name):
    z, frames, kinds, bnd = _case(name)
    F, N = frames.shape[:2]
    snaps, inv = _snaps(frames), _snaps(frames, slab=None)
    for mode in MODES:
        out, nF = snaps.global_step(kinds, float(z["dt"]), z["masses"], velocity=mode)
        assert nF == F and tuple(out.shape) == (F, N, 3) and out.is_cuda
        got = out.cpu().numpy()
        assert _report("%s %s slab (kappa %.3g)" % (name, mode, z["kappa"]), got, z["q_" + mode], bnd[mode]) <= bnd[mode]
        other = inv.global_step(kinds, float(z["dt"]), z["masses"], velocity=mode)[0].cpu().numpy()
        assert _report("%s %s slab against inverse" % (name, mode), got, other, 2 * bnd[mode]) <= 2 * bnd[mode]
    ns, largest = snaps.global_solve_slabs
    assert ns >= 4 and largest < N and snaps.global_solve_residual <= 64 * EPS * z["kappa"]
    assert abs(snaps.global_matrix.toarray() - z["A"]).max() <= 1e-13 * np.abs(z["A"]).max()
    # global_solve on the caller's tensor: the bits of the step's own solve
    rhs_dev = snaps.constraint_forces(kinds)[0]
    whole = snaps.global_solve(rhs_dev)
    import torch
    for a, b in ((0, 1), (63, 65), (5, 70)):
        assert torch.equal(snaps.global_solve(rhs_dev[a:b].contiguous()), whole[a:b])


@pytest.mark.parametrize("name", NAMES)
def test_solve_frames_under_slab_matches_the_reference_loop(name):
    z, frames, kinds, one = _case(name)
    p = load_golden("pdsolve_" + name)
    F = frames.shape[0]
    snaps = _snaps(frames)
    for mode in MODES:
        for K in KS:
            out, nF = snaps.solve_frames(kinds, float(z["dt"]), K, z["masses"], velocity=mode)
            B = bound_K(one[mode], K, float(p["amp_%s_%d" % (mode, K)]))
            assert nF == F and _report("%s %s K = %d slab" % (name, mode, K), out.cpu().numpy(), p["q_%s_%d" % (mode, K)], B) <= B
    assert snaps.global_solve_slabs[0] >= 4


@pytest.mark.parametrize("fixture", ["tets_deim", "tris_blocks"])
def test_reduced_and_hyper_solves_under_slab_match_the_host_model(fixture):
    c = rf_case(fixture)
    z = golden(c.kind)
    hc = host_case(c.kind)
    amps = load_golden("pdsolve_reduced_" + fixture)
    frames = c.g["frames"]
    F = frames.shape[0]
    dt, masses = float(z["dt"]), z["masses"]
    snaps = _snaps(frames)
    for m in (c.ms[0], c.ms[-1]):
        op = rf_operator(c, m)
        for mode in MODES:
            host = model(hc, range(F), mode, KS, reduced=(0, op))
            for K in KS:
                amp = float(amps["amp_%d_%s_%d" % (m, mode, K)])
                B = bound_K(_reduced_one(c, z, m, host[K]), K, amp)
                out = snaps.solve_frames([hyper_spec(c, m)], dt, K, masses, velocity=mode)[0]
                assert _report("%s m = %d %s K = %d reduced slab" % (fixture, m, mode, K), out.cpu().numpy(), host[K], B) <= B
                Bh = bound_K(hyper_one(c, z, m, op, host[K]), K, amp)
                for hyper in ("touched", "all"):
                    out = snaps.solve_frames([hyper_spec(c, m)], dt, K, masses, velocity=mode, hyper=hyper)[0]
                    assert _report("%s m = %d %s K = %d %s slab" % (fixture, m, mode, K, hyper), out.cpu().numpy(), host[K], Bh) <= Bh


@pytest.mark.parametrize("name", NAMES)
def test_rollout_under_slab_matches_the_reference(name):
    z, frames, kinds, one = _case(name)
    _against_reference(name, _snaps(frames), z, kinds, one, "slab")     # T in STEPS[name], K in {1, 3, 10}, both modes


def test_error_sweeps_under_slab_agree_with_the_inverse():
    """The four sweeps under "slab" against their "inverse" numbers.  Both solvers' tensors lie within the fixture's bound B of
    the exact iteration (the bounds of sections 2's tests, with the LARGEST amplification the fixtures store for this kind), so
    they differ by at most 2 B entrywise, and the Frobenius metric of (full, reduced) moves by at most the Frobenius norms of
    the two differences: 2 (2 B) sqrt(3 F N)."""
    c = rf_case("tris_blocks")
    z = golden(c.kind)
    frames = c.g["frames"]
    F, N = frames.shape[:2]
    dt, masses = float(z["dt"]), z["masses"]
    kw = dict(reduction=c.reduction, **_reduced_kw(c))
    slab, inv = _snaps(frames), _snaps(frames, slab=None)
    n = 3 * F * N
    rs = [c.ms[0], c.ms[-1]]
    q = z["q_difference"]
    one = max(_case(c.kind)[3]["difference"], max(_reduced_one(c, z, m, q) for m in rs))
    stored = [load_golden(f) for f in ("pdsolve_" + c.kind, "pdsolve_reduced_tris_blocks", "rollout_" + c.kind, "rollout_reduced_tris_blocks")]
    amp = max(float(v) for g in stored for k, v in g.items() if k.startswith("amp_"))
    assert 1.0 <= amp <= 1e3
    T, K = 2, 3
    calls = [("reduced_global_step_errors", lambda s: s.reduced_global_step_errors(c.kind, c.basis, rs, dt, masses, **kw), one),
             ("reduced_solve_errors", lambda s: s.reduced_solve_errors(c.kind, c.basis, rs, dt, K, masses, **kw), bound_K(one, K, amp)),
             ("reduced_solve_errors hyper", lambda s: s.reduced_solve_errors(c.kind, c.basis, rs, dt, K, masses, hyper="touched", **kw),
              bound_K(one, K, amp)),
             ("reduced_rollout_errors", lambda s: [v[:, -1] for v in s.reduced_rollout_errors(c.kind, c.basis, rs, dt, T, K, masses, **kw)[:5]],
              bound_T(one, K, T, amp, adv_bound(q, q)))]
    for tag, call, B in calls:
        a, b = call(slab), call(inv)
        allowed = 2 * (2 * B) * np.sqrt(n)
        for i, r in enumerate(rs):
            print("%s r = %d: fro %.12g (inverse %.12g), difference %.3g, allowed %.3g" % (tag, r, a[0][i], b[0][i], abs(a[0][i] - b[0][i]), allowed))
            assert abs(a[0][i] - b[0][i]) <= allowed
            assert np.isfinite([a[j][i] for j in range(5)]).all()
        assert abs(a[0][-1] - a[0][0]) > allowed                # not vacuous: the numbers of two r differ by more than that


# ------------------------------------------------------------------ 3. bit identity under "slab"
@pytest.mark.parametrize("name", ["tets_strain", "tris_strain", "combined"])
def test_repeats_ranges_chunks_and_continued_solves_are_bit_identical(name):
    import torch
    z, frames, kinds, _ = _case(name)
    dt, m = float(z["dt"]), z["masses"]
    snaps = _snaps(frames)
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
        # T1 + T2 time steps; one step is solve_frames(start="explicit")
        q3, p3, _ = snaps.simulate_frames(kinds, dt, 3, 2, m, velocity=mode, **SEL)
        q1, p1, _ = snaps.simulate_frames(kinds, dt, 1, 2, m, velocity=mode, **SEL)
        q2, p2, _ = snaps.simulate_frames(kinds, dt, 2, 2, m, state=(q1, p1), **SEL)
        assert torch.equal(q2, q3) and torch.equal(p2, p3)
        assert torch.equal(q1, snaps.solve_frames(kinds, dt, 2, m, velocity=mode, start="explicit", **SEL)[0])
    # switching to "inverse" and back: each solver reproduces its own bits, and the two differ only by rounding
    want = snaps.solve_frames(kinds, dt, 3, m)[0]
    snaps.set_global_solver("inverse")
    inv = snaps.solve_frames(kinds, dt, 3, m)[0]
    assert torch.equal(inv, _snaps(frames, slab=None).solve_frames(kinds, dt, 3, m)[0])
    snaps.set_global_solver("slab", TARGET)
    assert torch.equal(snaps.solve_frames(kinds, dt, 3, m)[0], want)
    assert float((inv - want).abs().max()) <= 1e-9 * float(want.abs().max())


@pytest.mark.parametrize("fixture", ["tets_deim", "tris_blocks"])
def test_hyper_identities_under_slab(fixture):
    c = rf_case(fixture)
    z = golden(c.kind)
    snaps = _snaps(c.g["frames"])
    _identities(snaps, hyper_spec(c, c.ms[-1]), float(z["dt"]), z["masses"], c.g["frames"].shape[0])     # "touched" = "all", repeats, ranges, chunks, K + L


def test_a_solve_after_one_of_another_shape_equals_a_fresh_context():
    import torch
    frames, kinds, m, dt = _mesh("chain33")
    fresh = _snaps(frames[:20]).solve_frames(kinds, dt, 3, m)[0]
    big_frames, big_kinds, big_m, big_dt = _mesh("stiff")
    big = _snaps(big_frames[:70], slab=16)
    big.solve_frames(big_kinds, big_dt, 2, big_m)
    small = _snaps(frames[:20], engine=big._engine)
    assert small._engine is big._engine
    assert torch.equal(small.solve_frames(kinds, dt, 3, m)[0], fresh)


# ------------------------------------------------------------------ 4. the lifted limit
def test_a_chain_of_50001_vertices():
    import torch
    from animsnapbases_amd import _lib, projections as proj
    n, F = 50001, 3
    rest, edges, m = chain(n)
    frames = animate(rest, F, seed=8)
    dt, wi = 0.25, 2.0
    kinds = [dict(kind="edge_spring", elements=edges, wi=wi, rest_positions=rest)]
    snaps = _snaps(frames, slab=512)
    snaps.global_solve_setup(kinds, dt, m)
    A = snaps.global_matrix
    assert snaps.global_solve_slabs == (98, 512)
    kappa = gershgorin_kappa(A)
    assert snaps.global_solve_residual <= 64 * EPS * kappa
    # global_solve against the refined host solution
    B = rhs(n, 3 * F, 5)
    ref = np.asarray(refined_solve(A, B), dtype=np.float64).reshape(n, F, 3).transpose(1, 0, 2)
    dev = torch.from_numpy(np.ascontiguousarray(B.reshape(n, F, 3).transpose(1, 0, 2))).to("cuda:%d" % snaps._engine.device_id)
    bnd = bound(kappa, ref)
    assert _report("chain 50001 global_solve (kappa <= %.3g)" % kappa, snaps.global_solve(dev).cpu().numpy(), ref, bnd) <= bnd
    # one global_step against splu: the bound of tests/gstep_cases.py with || |A^-1| ||_inf <= 1 / min_i (a_ii - sum_{j != i} |a_ij|)
    setup = proj.build_setup("edge_spring", edges, rest)
    St = proj.assembly_ST(setup, n, wi)
    p = proj.project_host(setup, frames, 1.0, 1.0)
    s = 2.0 * frames - frames[[0, 0, 1]]
    b = np.stack([St @ p[f] for f in range(F)]) + (m / dt ** 2)[None, :, None] * s
    q = np.asarray(refined_solve(A, b.transpose(1, 0, 2).reshape(n, 3 * F)), dtype=np.float64).reshape(n, F, 3).transpose(1, 0, 2)
    ln = np.linalg.norm(frames[:, edges[:, 1]] - frames[:, edges[:, 0]], axis=2)
    d = np.linalg.norm(rest[edges[:, 1]] - rest[edges[:, 0]], axis=1)
    tol_p = 64 * EPS * np.abs(frames).max() / ln.min() * max(1.0, (d[None] / ln).max())
    diag = A.diagonal()
    ainv_inf = 1.0 / (2 * diag - np.asarray(abs(A).sum(axis=1)).ravel()).min()
    bnd = ainv_inf * force_bound(St, p, tol_p).max() + 64 * EPS * kappa * np.abs(q).max()
    out, nF = snaps.global_step(kinds, dt, m, velocity="difference")
    assert nF == F and _report("chain 50001 global_step", out.cpu().numpy(), q, bnd) <= bnd
    # the same object under "inverse" still refuses the size
    snaps.set_global_solver("inverse")
    with pytest.raises(RuntimeError, match="46000"):
        snaps.global_solve_setup(kinds, dt, m)
    eng = snaps._engine
    one = np.zeros(1, dtype=np.int64)
    assert eng.lib.asb_gstep_setup(eng.h, n, _lib.ptr(one), None, None, None) == _lib.ERR_LIMIT
    with pytest.raises(ValueError, match="global_solve_setup"):     # the refused set-up left no solver, and released the factor
        snaps.global_solve(dev)


# ------------------------------------------------------------------ 5. refusals
def test_refusals_at_the_c_entry():
    import torch
    from animsnapbases_amd import _lib, projections as proj
    n = 33
    A = chain_matrix(n)
    eng = _engine(n)
    plan = proj.slab_plan(A, 4)
    good = torch.zeros((4, n, 3), dtype=torch.float64, device="cuda:%d" % eng.device_id)
    out = torch.empty_like(good)
    ns = types.SimpleNamespace

    def no_solver():
        with pytest.raises(RuntimeError, match="asb_gstep_setup"):
            eng.gstep_run(good.data_ptr(), 4, out.data_ptr())
        assert eng.gslab_held(A, plan) is None

    twice = plan.order.copy()
    twice[5] = twice[6]
    far = plan.order.copy()
    far[[0, n - 1]] = far[[n - 1, 0]]                       # the chain's two ends change places: slab 0 couples to the last
    cases = [(ns(order=twice, slab_ptr=plan.slab_ptr), "not a permutation"),
             (ns(order=plan.order + 1, slab_ptr=plan.slab_ptr), "not a permutation"),
             (ns(order=plan.order, slab_ptr=np.r_[plan.slab_ptr[:-1], n - 1]), "do not cover"),
             (ns(order=plan.order, slab_ptr=np.r_[1, plan.slab_ptr[1:]]), "do not cover"),
             (ns(order=plan.order, slab_ptr=np.r_[plan.slab_ptr[:2], plan.slab_ptr[1:]]), "do not cover"),
             (ns(order=far, slab_ptr=plan.slab_ptr), "not block tridiagonal")]
    for bad, what in cases:
        eng.gslab_setup(A, plan)                            # a factor is there ...
        eng.gstep_run(good.data_ptr(), 4, out.data_ptr())
        with pytest.raises(RuntimeError, match=what):
            eng.gslab_setup(A, bad)
        no_solver()                                         # ... and a refused set-up leaves none
    # the matrix checks of asb_gstep_setup, under this entry's name
    for broken, what in ((A[:-1, :-1].tocsr(), "rows"), (sparse.triu(A).tocsr(), "symmetric")):
        with pytest.raises(RuntimeError, match=what):
            eng.gslab_setup(broken, plan)
        assert b"asb_gslab_setup" in eng.lib.asb_last_error(eng.h)
        no_solver()
    # counts before pointers: nothing behind them is read
    one = np.zeros(1, dtype=np.int64)
    assert eng.lib.asb_gslab_setup(eng.h, n, _lib.ptr(one), None, None, 0, _lib.ptr(one), _lib.ptr(one), None) == _lib.ERR_ARG
    assert eng.lib.asb_gslab_setup(eng.h, n, _lib.ptr(one), None, None, n + 1, _lib.ptr(one), _lib.ptr(one), None) == _lib.ERR_ARG
    # a Schur complement that is not positive definite: that call's error, no solver
    indef = (A - sparse.diags(np.where(np.arange(n) == plan.order[n // 2], 0.999 * A.diagonal(), 0.0))).tocsr()
    with pytest.raises(RuntimeError, match="positive definite"):
        eng.gslab_setup(indef, plan)
    no_solver()
    # under the factor: the inverse's hook and the history are refused
    eng.gslab_setup(A, plan)
    assert eng.lib.asb_test_gstep_inverse(eng.h, _lib.ptr(np.empty((n, n))), n) == _lib.ERR_ARG
    frames, kinds, m, dt = _mesh("chain33")
    snaps = _snaps(frames[:5])
    snaps.solve_frames(kinds, dt, 1, m)
    e2 = snaps._engine
    assert e2.lib.asb_pdsolve_iterate(e2.h, 1, 0, None, _lib.ptr(np.empty((1, 5, 2)))) == _lib.ERR_ARG
    assert b"history" in e2.lib.asb_last_error(e2.h)
    with pytest.raises(ValueError, match="history"):
        snaps.solve_frames(kinds, dt, 2, m, history=True)
    # the other way round: the inverse's set-up releases the factor
    e2.gstep_setup(snaps.global_matrix)
    assert e2.gslab_held(snaps.global_matrix, proj.slab_plan(snaps.global_matrix, TARGET)) is None
    with pytest.raises(RuntimeError, match="no slab factor"):
        e2.gslab_info()
