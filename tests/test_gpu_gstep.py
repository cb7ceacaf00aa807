"""GPU (-m gpu): the global step of projective dynamics on a resident animation -- asb_gstep_setup / asb_gstep_run /
asb_gstep_inertia of csrc/asb_gstep.hip and posSnapshots.global_solve_setup / global_solve / global_step /
reduced_global_step_errors -- against the fixtures the UNMODIFIED reference wrote (tools/gen_golden_gstep.py: the triplets of
get_wi_SiT_AiT_Ai_Si assembled as Simulators.py:141-142, q = factorized(A_3)(b + M / h^2 s), wi = 0.7, dt = 0.5).

Shapes.  k_gstep_gemm's tile is 64 frames (16 per wave) x 32 vertices, its contraction runs in LDS stages of 16 vertices:
N in {1, 15, 16, 17, 31, 32, 33, 65, 100} x F' in {1, 63, 64, 65, 130}.  The golden meshes have 18 and 42 vertices, the
synthetic stiff one 100.

Bounds: tests/gstep_cases.py derives them (product kernel: (N + 4) eps sum |rhs| |A^-1| against a longdouble sum of the device's
own inverse; step: || |A^-1| ||_inf (force bound of tests/test_gpu_cforces.py) + 64 eps kappa(A) max |q|; set-up:
64 eps kappa(A)).  Every measured error is printed beside its bound.  Bit-identity claims are checked with torch.equal."""
import contextlib
import io

import numpy as np
import pytest
from scipy import sparse
from scipy.sparse.linalg import splu

from conftest import load_golden
from gstep_cases import EPS, KINDS, golden, product_model, spd_band, stiff_case, step_bound
from reduced_forces_cases import bound as rf_bound, case as rf_case, operator as rf_operator
from test_gpu_cforces import _bound as force_bound, _g, _spec
from test_gpu_cproj import RAW_TOL, _kappa, _min_edge

pytestmark = pytest.mark.gpu

MODES = ["zero", "difference"]


def _snaps(frames, standarize=False, mass=None, test_verts=None):
    from animsnapbases_amd import posSnapshots
    with contextlib.redirect_stdout(io.StringIO()):
        return posSnapshots.from_arrays(np.array(frames), None, "first", standarize=standarize, massWeight=mass is not None,
                                        mass=mass, test_verts=test_verts)


def _case(name, tol_p=RAW_TOL):
    """(fixture, frames, kinds, per-mode bound) of a golden kind or of "combined" (edges + tetrahedra on the latter's frames)."""
    z = golden(name)
    if name == "combined":
        ge, _, St_e = _g("edge_spring")
        gt, _, St_t = _g("tets_strain")
        c = load_golden("st_combined")
        fb = force_bound(St_e, c["p_edge"], tol_p) + force_bound(St_t, gt["expected"], tol_p)
        return z, gt["frames"], [_spec("edge_spring"), _spec("tets_strain")], step_bound(z, fb)
    g, _, St = _g(name)
    return z, g["frames"], [_spec(name)], step_bound(z, force_bound(St, g["expected"], tol_p))


def _report(tag, got, ref, bnd):
    err = np.abs(got - ref).max()
    print("%s: max abs err %.3g, bound %.3g, err / bound %.3g" % (tag, err, bnd, err / bnd))
    return err


# ------------------------------------------------------------------ 1. the product kernel alone
@pytest.mark.parametrize("N", [1, 15, 16, 17, 31, 32, 33, 65, 100])
def test_product_kernel_against_longdouble(N):
    import torch
    rng = np.random.default_rng(100 + N)
    snaps = _snaps(rng.standard_normal((2, N, 3)))
    eng = snaps._engine
    A = spd_band(N, rng)
    eng.gstep_setup(A)
    Ainv = eng.gstep_inverse(N)
    assert np.isfinite(Ainv).all()
    for F in (1, 63, 64, 65, 130):
        rhs = rng.standard_normal((F, N, 3)) * 10.0 ** rng.integers(-3, 4, size=(F, N, 1))
        dev = torch.from_numpy(rhs).to("cuda:%d" % eng.device_id)
        out = torch.full_like(dev, float("nan"))
        torch.cuda.synchronize()                    # the fill is on torch's stream, the product on the engine's own
        eng.gstep_run(dev.data_ptr(), F, out.data_ptr())
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.isfinite(got).all(), (N, F)                       # every entry was overwritten
        assert torch.equal(dev.cpu(), torch.from_numpy(rhs))        # the operand was not touched
        ref, mag = product_model(rhs, Ainv)
        bnd = (N + 4) * EPS * mag
        err = np.abs((got.astype(np.longdouble) - ref).astype(np.float64))
        print("N = %d F' = %d: largest err / bound %.3g" % (N, F, (err / bnd).max()))
        assert (err <= bnd).all(), (N, F)


# ------------------------------------------------------------------ 2. the set-up on a stiff matrix
def test_setup_of_a_stiff_matrix():
    c = stiff_case()
    N, kappa = c["rest"].shape[0], c["kappa"]
    snaps = _snaps(c["rest"][None])
    snaps.global_solve_setup([dict(kind="tets_strain", elements=c["tets"], wi=c["wi"], rest_positions=c["rest"])], c["dt"], c["masses"])
    assert abs(snaps.global_matrix - c["A"]).max() == 0.0 and snaps.global_matrix.has_sorted_indices
    Ainv = snaps._engine.gstep_inverse(N)
    defect = np.abs(c["A"].toarray() @ Ainv - np.eye(N)).max()
    bnd = 64 * EPS * kappa
    print("kappa %.4g: |A A^-1 - I|_max %.3g (/ eps kappa: %.3g), residual %.3g (/ eps kappa: %.3g), bound %.3g"
          % (kappa, defect, defect / (EPS * kappa), snaps.global_solve_residual, snaps.global_solve_residual / (EPS * kappa), bnd))
    assert defect <= bnd
    assert 0.0 <= snaps.global_solve_residual <= bnd
    assert np.abs(Ainv - Ainv.T).max() <= bnd * np.abs(Ainv).max()
    # the residual is the one of the definition: A applied to the column sums of the device's inverse
    host = np.abs(c["A"] @ Ainv.sum(axis=0) - 1.0).max()
    assert abs(snaps.global_solve_residual - host) <= 4 * N * EPS * (abs(c["A"]) @ np.abs(Ainv).sum(axis=0)).max()


# ------------------------------------------------------------------ 3. one step of every golden kind, both velocity modes
@pytest.mark.parametrize("name", KINDS + ["combined"])
def test_global_step_matches_the_reference(name):
    z, frames, kinds, bnd = _case(name)
    F, N = frames.shape[:2]
    snaps = _snaps(frames)
    for mode in MODES:
        out, nF = snaps.global_step(kinds, float(z["dt"]), z["masses"], velocity=mode)
        assert nF == F and tuple(out.shape) == (F, N, 3) and str(out.dtype) == "torch.float64" and out.is_cuda
        err = _report("%s %s (kappa %.3g)" % (name, mode, z["kappa"]), out.cpu().numpy(), z["q_" + mode], bnd[mode])
        assert err <= bnd[mode]
    assert abs(snaps.global_matrix.toarray() - z["A"]).max() <= 1e-13 * np.abs(z["A"]).max()
    assert snaps.global_solve_residual <= 64 * EPS * z["kappa"]
    assert list(snaps.assembly_ST) == [k["kind"] for k in kinds]


@pytest.mark.parametrize("name", KINDS + ["combined"])
def test_weighted_standardised_tensor_and_heldout(name):
    kind = "tets_strain" if name == "combined" else name
    g = _g(kind)[0]
    if name == "combined":
        tol_p = 64 * EPS * np.abs(g["frames"]).max() * max(_kappa(k, _g(k)[0]) / _min_edge(k, _g(k)[0]) for k in ("edge_spring", "tets_strain"))
    else:
        tol_p = 64 * EPS * np.abs(g["frames"]).max() / _min_edge(kind, g) * _kappa(kind, g)
    z, frames, kinds, bnd = _case(name, tol_p)
    N = frames.shape[1]
    mass = 0.5 + np.random.default_rng(3).random(N)                 # the weighting of the tensor is not the solver's mass
    snaps = _snaps(frames, standarize=True, mass=mass)
    assert snaps.pre_scale_factor != 1 and snaps.massL is not None
    for mode in MODES:
        out, _ = snaps.global_step(kinds, float(z["dt"]), z["masses"], velocity=mode)
        err = _report("%s %s weighted" % (name, mode), out.cpu().numpy(), z["q_" + mode], bnd[mode])
        assert err <= bnd[mode]
    # the same frames as a held-out animation of snapshots trained on the first three; frame 13 of the fixture is frame 3 of
    # the held-out tensor, whose previous frame is the fixture's frame 12 whatever the jump
    snaps = _snaps(frames[:3], standarize=True, mass=mass)
    for mode in MODES:
        out, nF = snaps.global_step(kinds, float(z["dt"]), z["masses"], velocity=mode, animation=np.array(frames[10:]),
                                    frame_start=3, frame_jump=2, chunk_frames=16)
        ref = z["q_" + mode][13::2]
        assert nF == ref.shape[0]
        err = _report("%s %s held-out" % (name, mode), out.cpu().numpy(), ref, bnd[mode])
        assert err <= bnd[mode]
    # no masses given: the ones the snapshots were weighted with
    snaps.global_solve_setup(kinds, 0.5)
    ref = z["A"] - np.diag(z["masses"] / 0.25) + np.diag(mass / 0.25)
    assert abs(snaps.global_matrix.toarray() - ref).max() <= 1e-13 * np.abs(ref).max()


# ------------------------------------------------------------------ 4. bit-identity
@pytest.mark.parametrize("name", ["tets_strain", "tris_strain"])
def test_repeats_ranges_and_chunks_are_bit_identical(name):
    import torch
    z, frames, kinds, _ = _case(name)
    snaps = _snaps(frames)
    dt, m = float(z["dt"]), z["masses"]
    full_zero = snaps.global_step(kinds, dt, m, velocity="zero")[0]
    for mode in MODES:
        full = snaps.global_step(kinds, dt, m, velocity=mode)[0]
        assert torch.equal(snaps.global_step(kinds, dt, m, velocity=mode)[0], full)
        part, nF = snaps.global_step(kinds, dt, m, velocity=mode, frame_start=3, frame_end=67, frame_jump=2)
        assert nF == 32 and torch.equal(part, full[3:67:2])
        assert torch.equal(snaps.global_step(kinds, dt, m, velocity=mode, chunk_frames=16)[0], full)
    # an unchanged matrix keeps the device's inverse; another time step replaces it
    eng, A = snaps._engine, snaps.global_matrix
    assert eng.gstep_held(A) == snaps.global_solve_residual and eng.gstep_held(A * 2.0) is None and eng.gstep_held(A[:-1, :-1]) is None
    calls = []
    eng.gstep_setup, real = (lambda M: calls.append(1) or real(M)), eng.gstep_setup
    snaps.global_solve_setup(kinds, dt, m)
    assert calls == []
    snaps.global_solve_setup(kinds, 2 * dt, m)
    assert calls == [1] and eng.gstep_held(A) is None and eng.gstep_held(snaps.global_matrix) is not None
    snaps.global_solve_setup(kinds, dt, m)
    assert calls == [1, 1] and torch.equal(snaps.global_step(kinds, dt, m, velocity="zero")[0], full_zero)
    rhs = snaps.constraint_forces(kinds)[0]
    whole = snaps.global_solve(rhs)
    assert torch.equal(snaps.global_solve(rhs), whole)
    for a, b in ((0, 1), (63, 65), (5, 70), (129, 130)):
        assert torch.equal(snaps.global_solve(rhs[a:b].contiguous()), whole[a:b]), (a, b)


def test_collapsed_edge_poisons_exactly_its_frame():
    g, s, _ = _g("edge_spring_collapsed")
    nan_frames = np.isnan(s["b"]).any(axis=(1, 2))
    assert nan_frames.tolist() == [False, False, True, False]
    N = g["rest"].shape[0]
    snaps = _snaps(g["frames"])
    for mode in MODES:
        out = snaps.global_step([_spec("edge_spring_collapsed")], 0.5, np.ones(N), velocity=mode)[0].cpu().numpy()
        # A^-1 is dense: the NaN of the two vertices reaches every vertex of that frame, and no other frame
        assert np.isnan(out[nan_frames]).all() and np.isfinite(out[~nan_frames]).all()


# ------------------------------------------------------------------ 5. the inertia term
def _host_inertia(frames, sel, diag, mode, acc):
    prev = frames[[max(f - 1, 0) for f in sel]]
    s = frames[list(sel)] if mode == 0 else 2.0 * frames[list(sel)] - prev
    return diag[None, :, None] * (s + acc[None, None, :])


@pytest.mark.parametrize("weighted", [False, True])
def test_inertia_kernel_against_the_host_formula(weighted):
    import torch
    g = _g("tets_strain")[0]
    frames = g["frames"]
    F, N = frames.shape[:2]
    mass = 0.5 + np.random.default_rng(5).random(N) if weighted else None
    snaps = _snaps(frames, standarize=weighted, mass=mass)
    eng = snaps._engine
    diag = (0.3 + np.random.default_rng(6).random(N)) / 0.01
    # positions come back from the tensor with four roundings each on the weighted path, none on the raw one; the formula adds
    # at most three more on either side
    tol = (16 if weighted else 4) * EPS
    for mode in (0, 1):
        for acc in (np.zeros(3), np.array([0.0, -0.0981, 0.02])):
            for f0, f1, fj in ((0, F, 1), (0, 1, 1), (3, 67, 2), (63, 66, 1), (1, F, 64)):
                sel = range(f0, f1, fj)
                base = np.random.default_rng(7).standard_normal((len(sel), N, 3))
                buf = torch.from_numpy(base).to("cuda:%d" % eng.device_id)
                eng.gstep_inertia(0, f0, f1, fj, snaps.invMassL, snaps._standarize, snaps.pre_scale_factor, diag, mode, acc, buf.data_ptr())
                add = _host_inertia(frames, sel, diag, mode, acc)
                size = diag[None, :, None] * (3.0 * np.abs(frames).max() + np.abs(acc).max()) + np.abs(base)
                err = np.abs(buf.cpu().numpy() - (base + add))
                assert (err <= tol * size).all(), (mode, f0, f1, fj, (err / size).max() / EPS)
    # frame 0 has no previous frame: x_{-1} = x_0 and 2 x - x = x exactly, so both modes give the bits of s = x
    a = torch.zeros((1, N, 3), dtype=torch.float64, device="cuda:%d" % eng.device_id)
    b = torch.zeros_like(a)
    eng.gstep_inertia(0, 0, 1, 1, snaps.invMassL, snaps._standarize, snaps.pre_scale_factor, diag, 0, np.zeros(3), a.data_ptr())
    eng.gstep_inertia(0, 0, 1, 1, snaps.invMassL, snaps._standarize, snaps.pre_scale_factor, diag, 1, np.zeros(3), b.data_ptr())
    assert torch.equal(a, b)


def test_velocity_modes_and_gravity_of_the_public_step():
    import torch
    z, frames, kinds, bnd = _case("tets_strain")
    F, N = frames.shape[:2]
    dt, m = float(z["dt"]), z["masses"]
    lu = splu(sparse.csc_matrix(z["A"]))
    snaps = _snaps(frames)
    zero = snaps.global_step(kinds, dt, m, velocity="zero")[0]
    diff = snaps.global_step(kinds, dt, m, velocity="difference")[0]
    assert torch.equal(zero[0], diff[0]) and not torch.equal(zero[1:], diff[1:])            # the rule at frame 0
    # q_difference - q_zero = A^-1 M / h^2 (x_f - x_{f-1}): the constraint term drops out
    dx = frames - frames[[max(f - 1, 0) for f in range(F)]]
    ref = np.stack([lu.solve((m / dt ** 2)[:, None] * dx[f]) for f in range(F)])
    tol = 2 * 64 * EPS * z["kappa"] * max(np.abs(z["q_zero"]).max(), np.abs(z["q_difference"]).max())
    err = _report("difference - zero", (diff - zero).cpu().numpy(), ref, tol)
    assert err <= tol
    # gravity: q(g) - q(0) = A^-1 M g, the same for every frame
    grav = np.array([0.0, -9.81, 0.5])
    with_g = snaps.global_step(kinds, dt, m, velocity="zero", gravity=grav)[0]
    ref = lu.solve(m[:, None] * grav[None, :])
    tol = 2 * 64 * EPS * z["kappa"] * (np.abs(z["q_zero"]).max() + np.abs(ref).max())
    err = _report("gravity", (with_g - zero).cpu().numpy(), np.broadcast_to(ref, (F, N, 3)), tol)
    assert err <= tol and np.abs(ref).max() > 0.1


# ------------------------------------------------------------------ 6. the error of the reduced step against the host route
def test_reduced_global_step_errors_against_the_host_route():
    from animsnapbases_amd import constraintsComponents as cc
    c = rf_case("tets_deim")
    z = golden("tets_strain")
    frames = c.g["frames"]
    F, N = frames.shape[:2]
    dt, m = float(z["dt"]), z["masses"]
    kw = dict(elements=c.g["elements"], wi=0.7, reduction=c.reduction, rest_positions=c.g["rest"], sigma_min=c.g["sigma"][0],
              sigma_max=c.g["sigma"][1])
    snaps = _snaps(frames)
    rs = c.ms
    got = snaps.reduced_global_step_errors(c.kind, c.basis, rs, dt, m, per_frame=True, **kw)
    assert got[5].shape == (len(rs), F) and all(len(v) == len(rs) for v in got[:5])
    lu = splu(sparse.csc_matrix(snaps.global_matrix))
    b = snaps.constraint_forces([_spec("tets_strain")])[0].cpu().numpy()
    inertia = _host_inertia(frames, range(F), m / dt ** 2, 1, np.zeros(3))
    q = np.stack([lu.solve(b[f] + inertia[f]) for f in range(F)])
    fb = force_bound(_g("tets_strain")[2], c.g["expected"], RAW_TOL).max()
    n = 3 * F * N
    for i, r in enumerate(rs):
        bt = snaps.reduced_constraint_forces(c.kind, c.basis, r, **kw)[0].cpu().numpy()
        qt = np.stack([lu.solve(bt[f] + inertia[f]) for f in range(F)])
        # each device tensor is within B of the host's; the metrics are Lipschitz in their two arguments
        B = z["Ainv_abs_inf"] * max(fb, rf_bound(c, r, rf_operator(c, r)).max()) + 64 * EPS * z["kappa"] * np.abs(q).max()
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
    # a sweep equals single calls; nothing depends on the order
    single = snaps.reduced_global_step_errors(c.kind, c.basis, [rs[1]], dt, m, **kw)
    assert [v[0] for v in single] == [got[j][1] for j in range(5)]
    assert snaps.reduced_global_step_errors(c.kind, c.basis, [], dt, m, **kw) == ([], [], [], [], [])


# ------------------------------------------------------------------ 7. refusals
def test_refusals():
    import torch
    from animsnapbases_amd import _lib
    z, frames, kinds, _ = _case("tets_strain")
    F, N = frames.shape[:2]
    snaps = _snaps(frames)
    eng = snaps._engine
    dev = "cuda:%d" % eng.device_id
    good = torch.zeros((4, N, 3), dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="global_solve_setup"):
        snaps.global_solve(good)
    with pytest.raises(RuntimeError, match="asb_gstep_setup"):
        eng.gstep_run(good.data_ptr(), 4, torch.empty_like(good).data_ptr())
    with pytest.raises(ValueError, match="masses"):
        snaps.global_solve_setup(kinds, 0.5)                        # snapshots built without mass weighting
    snaps.global_solve_setup(kinds, float(z["dt"]), z["masses"])
    assert tuple(snaps.global_solve(good).shape) == (4, N, 3)
    for bad in (torch.zeros((4, N, 3), dtype=torch.float32, device=dev), torch.zeros((4, N + 1, 3), dtype=torch.float64, device=dev),
                torch.zeros((4, N), dtype=torch.float64, device=dev), torch.zeros((0, N, 3), dtype=torch.float64, device=dev),
                torch.zeros((4, N, 3), dtype=torch.float64), torch.zeros((4, 3, N), dtype=torch.float64, device=dev).transpose(1, 2),
                np.zeros((4, N, 3))):
        with pytest.raises(ValueError, match="global_solve"):
            snaps.global_solve(bad)
    with pytest.raises(RuntimeError, match="overlap"):
        eng.gstep_run(good.data_ptr(), 4, good.data_ptr())
    with pytest.raises(RuntimeError, match="overlap"):
        eng.gstep_run(good.data_ptr(), 2, good[1:].data_ptr())
    with pytest.raises(RuntimeError, match="frames"):
        eng.gstep_run(good.data_ptr(), 0, torch.empty_like(good).data_ptr())
    # a matrix that is no system matrix of this tensor
    A = snaps.global_matrix
    for broken, what in ((A[:-1, :-1].tocsr(), "rows"), ((A - sparse.diags(A.diagonal() * 2)).tocsr(), "diagonal"),
                         (sparse.triu(A).tocsr(), "symmetric"), ((A + sparse.triu(A, 1) * 1e-9).tocsr(), "symmetric")):
        with pytest.raises(RuntimeError, match=what):
            eng.gstep_setup(broken)
        assert eng.gstep_held(A) is None and "S^T" not in eng.lib.asb_last_error(eng.h).decode()
        with pytest.raises(RuntimeError, match="asb_gstep_setup"):  # a failed set-up leaves no inverse behind
            eng.gstep_run(good.data_ptr(), 4, torch.empty_like(good).data_ptr())
    # N above the limit, at the C entry: the count alone is refused, nothing behind the pointers is read
    one = np.zeros(1, dtype=np.int64)
    rc = eng.lib.asb_gstep_setup(eng.h, 46001, _lib.ptr(one), None, None, None)
    assert rc == _lib.ERR_LIMIT and b"46000" in eng.lib.asb_last_error(eng.h)
    with pytest.raises(ValueError, match="velocity"):
        snaps.global_step(kinds, 0.5, z["masses"], velocity="leapfrog")
    with pytest.raises(ValueError, match="gravity"):
        snaps.global_step(kinds, 0.5, z["masses"], gravity=(0.0, 1.0))
    with pytest.raises(ValueError, match="empty frame range"):
        snaps.global_step(kinds, 0.5, z["masses"], frame_start=F)
