"""GPU (-m gpu): the hyper-reduced solver iterations -- asb_hyper_operator / asb_hyper_iterate of csrc/asb_pdsolve.hip and
``posSnapshots.solve_frames(..., hyper=)`` / ``reduced_solve_errors(..., hyper=)`` -- against the host model of
tests/pdsolve_cases.py (never against the device's own path without the operator), bit for bit against themselves
("touched" against "all", repeats, frame sub-ranges, chunks, continued solves, a fresh context), and on edge-spring chains
against the NumPy affine form c + G coef of tests/hyper_cases.py evaluated from the device's own previous iterate.

Shapes.  k_hyper_apply's tile is 32 vertices x 64 frames, its contraction runs in steps of 4 basis vectors, the compact
iterate has N_t rows padded to 32 in G: the goldens (N = 18, 42; N_t < N) and chains of N in {2, 15, 16, 17, 31, 32, 33, 65}
(N_t < 32, N_t > 32 and ragged, N_t = N), each at F' in {1, 63, 64, 65, 130} and m in {1, 3, 4, 17} where the chain allows.

Bounds: B_K = 2 K max(1, amp) one_bound (tests/hyper_cases.py: the reduced one-iteration bound with N more terms in the
dot-product length for the sum that forms G), amp as stored with tests/golden/pdsolve_reduced_*.npz.  No frame is left out.
Every measured error is printed beside its bound."""
import contextlib
import io

import numpy as np
import pytest

from conftest import load_golden
from gstep_cases import EPS, golden
from hyper_cases import CHAINS, FRAMES, RAW_TOL, affine_parts, affine_step, chain_case, coefficients, one_bound, sampled
from pdsolve_cases import KS, MODES, bound_K, host_case, model
from reduced_forces_cases import case as rf_case, operator as rf_operator
from test_gpu_cforces import _bound as force_bound, _g

pytestmark = pytest.mark.gpu
_worst = {}


def _snaps(frames, engine=None):
    from animsnapbases_amd import posSnapshots
    kw = {} if engine is None else dict(engine=engine)
    with contextlib.redirect_stdout(io.StringIO()):
        return posSnapshots.from_arrays(np.array(frames), None, "first", standarize=False, massWeight=False, **kw)


def _kw(c):
    return dict(elements=c.g["elements"], wi=0.7, rest_positions=c.g["rest"], sigma_min=c.g["sigma"][0], sigma_max=c.g["sigma"][1])


def _spec(c, m):
    return dict(kind=c.kind, basis=c.basis, num_components=m, reduction=c.reduction, **_kw(c))


def _one(c, z, m, op, q):
    fb = force_bound(_g(c.kind)[2], c.g["expected"], RAW_TOL).max()
    return one_bound(z["Ainv_abs_inf"], z["kappa"], c.St, op, c.p_pt(m), c.r["cond_%d" % m], fb, RAW_TOL, np.abs(q).max())


# ------------------------------------------------------------------ 1. accuracy on the goldens, against the host model
@pytest.mark.parametrize("fixture", ["tets_deim", "tris_blocks"])
def test_hyper_solve_matches_the_host_model(fixture):
    c = rf_case(fixture)
    z = golden(c.kind)
    hc = host_case(c.kind)
    amps = load_golden("pdsolve_reduced_" + fixture)
    frames = c.g["frames"]
    F, N = frames.shape[:2]
    dt, masses = float(z["dt"]), z["masses"]
    snaps = _snaps(frames)
    assert amps["ms"].tolist() == [c.ms[0], c.ms[-1]]
    worst, coarse, last = 0.0, None, None
    for m in (c.ms[0], c.ms[-1]):
        op = rf_operator(c, m)
        for mode in MODES:
            host = model(hc, range(F), mode, KS, reduced=(0, op))
            for K in KS:
                B = bound_K(_one(c, z, m, op, host[K]), K, float(amps["amp_%d_%s_%d" % (m, mode, K)]))
                for hyper in ("touched", "all"):
                    out, nF = snaps.solve_frames([_spec(c, m)], dt, K, masses, velocity=mode, hyper=hyper)
                    assert nF == F and tuple(out.shape) == (F, N, 3) and str(out.dtype) == "torch.float64" and out.is_cuda
                    err = np.abs(out.cpu().numpy() - host[K]).max()             # every frame
                    print("%s m = %d %s K = %d %s: max abs err %.3g, B_K %.3g, err / B_K %.3g" % (fixture, m, mode, K, hyper, err, B, err / B))
                    worst = max(worst, err / B)
                    assert err <= B
                    if coarse is None and K == 10:
                        coarse, last = out.cpu().numpy(), B                     # (smallest m, velocity "zero")
    print("%s: largest err / B_K %.3g" % (fixture, worst))
    # the reduced term differs from the full one: the comparison above is not vacuous
    full = snaps.solve_frames([dict(kind=c.kind, **_kw(c))], dt, 10, masses, velocity="zero")[0].cpu().numpy()
    assert np.abs(full - coarse).max() > last


# ------------------------------------------------------------------ 2. bit identity
def _identities(snaps, spec, dt, masses, F, K=3):
    """"touched" = "all"; repeats, a sub-range, chunks of 16 frames; K iterations continued by L = K + L."""
    import torch
    kw = dict(frame_end=F)
    t = snaps.solve_frames([spec], dt, K, masses, hyper="touched", **kw)[0]
    a = snaps.solve_frames([spec], dt, K, masses, hyper="all", **kw)[0]
    assert torch.isfinite(t).all() and torch.equal(t, a)
    assert torch.equal(snaps.solve_frames([spec], dt, K, masses, hyper="touched", **kw)[0], t)
    assert torch.equal(snaps.solve_frames([spec], dt, K, masses, hyper="touched", chunk_frames=16, **kw)[0], t)
    assert torch.equal(snaps.solve_frames([spec], dt, K, masses, hyper="all", chunk_frames=16, **kw)[0], t)
    if F > 3:
        part, nF = snaps.solve_frames([spec], dt, K, masses, hyper="touched", frame_start=1, frame_end=F, frame_jump=2)
        assert nF == len(range(1, F, 2)) and torch.equal(part, t[1:F:2])
    for k, l in ((1, 2), (2, 1)):
        first = snaps.solve_frames([spec], dt, k, masses, hyper="touched", **kw)[0]
        keep = first.clone()
        assert torch.equal(snaps.solve_frames([spec], dt, l, masses, start=first, hyper="all", **kw)[0], t)
        assert torch.equal(snaps.solve_frames([spec], dt, l, masses, start=first, hyper="touched", **kw)[0], t)
        assert torch.equal(first, keep)
    return t


@pytest.mark.parametrize("fixture", ["tets_deim", "tris_blocks"])
def test_bit_identity_on_the_goldens(fixture):
    import torch
    c = rf_case(fixture)
    z = golden(c.kind)
    snaps = _snaps(c.g["frames"])
    F = c.g["frames"].shape[0]
    outs = [_identities(snaps, _spec(c, m), float(z["dt"]), z["masses"], F) for m in (c.ms[0], c.ms[-1])]
    assert not torch.equal(outs[0], outs[1])
    # the iterations move: K = 1 is not K = 3
    assert not torch.equal(snaps.solve_frames([_spec(c, c.ms[-1])], float(z["dt"]), 1, z["masses"], hyper="touched")[0], outs[1])


@pytest.mark.parametrize("n", CHAINS)
def test_chains_bit_identity_and_the_affine_form(n):
    c = chain_case(n)
    snaps = _snaps(c["frames"])
    worst = 0.0
    for m in c["ms"]:
        op = c["op"](m)
        spec = dict(c["spec"], basis=c["basis"], num_components=m)
        nt = sampled(c, op)[0].shape[0]
        for F in FRAMES:
            q3 = _identities(snaps, spec, c["dt"], c["masses"], F).cpu().numpy()
            # one iteration of the NumPy affine form from the DEVICE's own iterate after two
            q2 = snaps.solve_frames([spec], c["dt"], 2, c["masses"], frame_end=F, hyper="all")[0].cpu().numpy()
            want = affine_step(c, op, q2, affine_parts(c, op, range(F), "difference"))
            B = one_bound(c["Ainv_abs_inf"], c["kappa"], c["St"], op, coefficients(c, op, q2)[1], op.cond, 0.0, RAW_TOL, np.abs(want).max())
            err = np.abs(q3 - want).max()
            worst = max(worst, err / B)
            assert err <= B, (n, m, F, err, B)
        print("chain %d, m = %d (rpp %d), N_t = %d: largest err / one-iteration bound so far %.3g" % (n, m, (m + 3) // 4 * 4, nt, worst))


def test_a_hyper_solve_after_one_of_another_shape_equals_a_fresh_context():
    import torch
    small, big = chain_case(33), chain_case(65)
    spec = lambda c, m: dict(c["spec"], basis=c["basis"], num_components=m)
    fresh = _snaps(small["frames"][:70]).solve_frames([spec(small, 4)], small["dt"], 3, small["masses"], hyper="touched")[0]
    first = _snaps(big["frames"][:5])
    first.solve_frames([spec(big, 17)], big["dt"], 2, big["masses"], hyper="touched")
    again = _snaps(small["frames"][:70], engine=first._engine)
    assert again._engine is first._engine
    assert torch.equal(again.solve_frames([spec(small, 4)], small["dt"], 3, small["masses"], hyper="touched")[0], fresh)
    # on one tensor: a wide basis then a narrow one, many frames then few, the plain reduced path in between
    snaps = _snaps(big["frames"])
    want = _snaps(big["frames"]).solve_frames([spec(big, 3)], big["dt"], 2, big["masses"], frame_end=7, hyper="touched")[0]
    snaps.solve_frames([spec(big, 17)], big["dt"], 2, big["masses"], hyper="all")
    snaps.solve_frames([spec(big, 4)], big["dt"], 1, big["masses"])
    assert torch.equal(snaps.solve_frames([spec(big, 3)], big["dt"], 2, big["masses"], frame_end=7, hyper="touched")[0], want)


# ------------------------------------------------------------------ 3. reduced_solve_errors through the hyper path
def test_reduced_solve_errors_hyper_against_the_host_route():
    from animsnapbases_amd import constraintsComponents as cc
    c = rf_case("tets_deim")
    z = golden("tets_strain")
    hc = host_case("tets_strain")
    amps = load_golden("pdsolve_reduced_tets_deim")
    frames = c.g["frames"]
    F, N = frames.shape[:2]
    dt, masses, K = float(z["dt"]), z["masses"], 3
    kw = dict(reduction=c.reduction, **_kw(c))
    snaps = _snaps(frames)
    rs = [c.ms[0], c.ms[-1]]
    got = snaps.reduced_solve_errors(c.kind, c.basis, rs, dt, K, masses, per_frame=True, hyper="touched", **kw)
    assert got[5].shape == (len(rs), F) and all(len(v) == len(rs) for v in got[:5])
    q = model(hc, range(F), "difference", (K,))[K]
    amp_full = float(load_golden("pdsolve_tets_strain")["amp_difference_%d" % K])
    n = 3 * F * N
    for i, r in enumerate(rs):
        qt = model(hc, range(F), "difference", (K,), reduced=(0, rf_operator(c, r)))[K]
        B = bound_K(_one(c, z, r, rf_operator(c, r), q), K, max(amp_full, float(amps["amp_%d_difference_%d" % (r, K)])))
        e = q - qt
        fro, mx = cc.frobenius_error(q, qt), cc.max_pointwise_error(q, qt)
        rel = cc.relative_error_per_component(q, qt)
        slack = 1.0 + 4 * n * EPS
        print("r = %d: fro %.6g (host %.6g), max %.6g (host %.6g), B %.3g" % (r, got[0][i], fro, got[1][i], mx, B))
        assert abs(got[0][i] - fro) <= 2 * B * np.sqrt(n) * slack + 4 * n * EPS * fro
        assert abs(got[1][i] - mx) <= (2 * B + mx * B) / q.max() * slack * 2
        for d in range(3):
            nd = np.linalg.norm(q[:, :, d])
            assert abs(got[2 + d][i] - rel[d]) <= (2 * B + rel[d] * B) * np.sqrt(F * N) / nd * slack * 2 + 4 * n * EPS * rel[d]
        pf = np.linalg.norm(e.reshape(F, -1), axis=1) / np.linalg.norm(q.reshape(F, -1), axis=1)
        nf = np.linalg.norm(q.reshape(F, -1), axis=1)
        assert (np.abs(got[5][i] - pf) <= (2 * B + pf * B) * np.sqrt(3 * N) / nf * slack * 2 + 4 * n * EPS * pf).all()
    assert got[0][-1] < got[0][0]                                  # more components: a smaller error
    # a sweep equals single calls (G of the largest r serves the smaller r by its leading columns); "all" gives the same numbers
    for j, r in enumerate(rs):
        single = snaps.reduced_solve_errors(c.kind, c.basis, [r], dt, K, masses, hyper="touched", **kw)
        assert [v[0] for v in single] == [got[k][j] for k in range(5)]
    assert snaps.reduced_solve_errors(c.kind, c.basis, rs[::-1], dt, K, masses, hyper="all", **kw) == tuple(v[::-1] for v in got[:5])
    assert snaps.reduced_solve_errors(c.kind, c.basis, [], dt, K, masses, hyper="touched", **kw) == ([], [], [], [], [])


# ------------------------------------------------------------------ 4. NaN containment
def test_a_nan_frame_of_the_start_stays_in_its_frame():
    """On a chain: an edge spring's projection d s / |s| hands a NaN of the iterate on (the strain kinds' clamps, fmin / fmax,
    swallow one), so the frame's coefficients, and with them every row of the frame, are NaN -- and no other frame's."""
    c = chain_case(33)
    spec = dict(c["spec"], basis=c["basis"], num_components=4)
    snaps = _snaps(c["frames"])
    F = 70
    start = snaps.solve_frames([spec], c["dt"], 1, c["masses"], frame_end=F, hyper="all")[0]
    start[66] = float("nan")
    for hyper in ("touched", "all"):
        out = snaps.solve_frames([spec], c["dt"], 3, c["masses"], start=start, frame_end=F, hyper=hyper)[0].cpu().numpy()
        bad = np.isnan(out).any(axis=(1, 2))
        assert bad.tolist() == [f == 66 for f in range(F)] and np.isnan(out[66]).all() and np.isfinite(out[~bad]).all()


# ------------------------------------------------------------------ 5. refusals at both layers
def test_refusals():
    import torch
    from animsnapbases_amd import projections as proj
    c = rf_case("tets_deim")
    z = golden(c.kind)
    frames = c.g["frames"]
    N = frames.shape[1]
    dt, m = float(z["dt"]), z["masses"]
    snaps = _snaps(frames)
    eng = snaps._engine
    red, plain = _spec(c, c.ms[0]), dict(kind=c.kind, **_kw(c))
    with pytest.raises(ValueError, match="every kind reduced"):
        snaps.solve_frames([plain], dt, 1, m, hyper="touched")
    with pytest.raises(ValueError, match="exactly one kind"):
        snaps.solve_frames([red, dict(red, kind="tets_deformation_gradient")], dt, 1, m, hyper="touched")
    with pytest.raises(ValueError, match="history"):
        snaps.solve_frames([red], dt, 1, m, history=True, hyper="all")
    with pytest.raises(ValueError, match="hyper must be"):
        snaps.solve_frames([red], dt, 1, m, hyper="rows")
    with pytest.raises(RuntimeError, match="asb_gstep_setup"):      # nothing above reached the device: it holds no inverse
        eng.hyper_operator()
    good = snaps.solve_frames([red], dt, 2, m, frame_end=4, hyper="touched")[0]
    # ---- the C layer.  The solve above left the inverse, S^T V and G on the device
    op = rf_operator(c, c.ms[0])
    full = proj.build_setup(c.kind, c.g["elements"], c.g["rest"])
    touched, compact = proj.touched_setup(proj.subset_setup(full, op.elements))

    def begin(setup=compact, St=None):
        eng.pdsolve_begin(0, 0, 4, 1, None, False, 1.0, m / dt ** 2, 1, np.zeros(3), 0)
        eng.cproj_setup(setup)
        eng.rforce_solver(op.H, op.local_rows)
        eng.pdsolve_slot(c.g["sigma"][0], c.g["sigma"][1], St)
    out = torch.empty_like(good)
    begin()
    eng.hyper_iterate(2, touched, 0, out.data_ptr())
    assert torch.equal(out, good)
    begin()
    with pytest.raises(RuntimeError, match="ascending"):
        eng.hyper_iterate(1, touched[::-1])
    with pytest.raises(RuntimeError, match="names vertex"):         # the set-up is numbered into more rows than the iterate is given
        eng.hyper_iterate(1, touched[:-1])
    with pytest.raises(RuntimeError, match="touched vertices"):
        eng.hyper_iterate(1, np.arange(N + 1))
    with pytest.raises(RuntimeError, match="iterations"):
        eng.hyper_iterate(0, touched)
    begin(full, proj.assembly_ST(full, N, 0.7))                     # a kind that is not reduced
    with pytest.raises(RuntimeError, match="every kind must be reduced"):
        eng.hyper_iterate(1, touched)
    eng.pdsolve_begin(0, 0, 4, 1, None, False, 1.0, m / dt ** 2, 1, np.zeros(3), 0)
    with pytest.raises(RuntimeError, match="no kind registered"):
        eng.hyper_iterate(1, touched)
    # a stale G: another matrix, or another basis, between the operator and the solve -- an error, not a wrong result
    A = proj.global_matrix([(full, 0.7)], N, m, dt)
    eng.gstep_setup(proj.global_matrix([(full, 0.7)], N, m, 2 * dt))
    begin()
    with pytest.raises(RuntimeError, match="stale"):
        eng.hyper_iterate(1, touched)
    eng.gstep_setup(A)
    eng.hyper_operator()
    eng.rforce_operator(proj.assembly_ST(full, N, 0.7), op.V)
    begin()
    with pytest.raises(RuntimeError, match="stale"):
        eng.hyper_iterate(1, touched)
    eng.hyper_operator()
    begin()
    eng.hyper_iterate(2, touched, 0, out.data_ptr())
    assert torch.equal(out, good)                                   # and with G formed again, the same bits
    assert torch.equal(snaps.solve_frames([red], dt, 2, m, frame_end=4, hyper="all")[0], good)
