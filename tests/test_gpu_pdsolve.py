"""GPU (-m gpu): the solver iterations of projective dynamics on a resident animation -- asb_pdsolve_begin / _slot / _iterate of
csrc/asb_pdsolve.hip and posSnapshots.solve_frames / reduced_solve_errors -- against the fixtures of the UNMODIFIED reference's
own loop (tools/gen_golden_pdsolve.py: Simulators.py:506-526, wi = 0.7, dt = 0.5, K in {1, 3, 10}), against the host route of
tests/pdsolve_cases.py for the reduced kind, and bit for bit against ``global_step`` and against itself.

Shapes.  k_pdsolve_gemm's tile is 64 frames x 32 vertices, its contraction runs in stages of 16 vertices, the iterate's rows
are padded to 64 frames: the goldens (N = 18, 42), the stiff box (N = 100) and edge-spring chains of N in {2, 15, 16, 17, 31,
32, 33, 65} vertices, each at F' in {1, 63, 64, 65, 130}.

Bounds: B_K = 2 K max(1, amp) (one-iteration bound), amp measured on the host model and stored with the fixtures
(tests/pdsolve_cases.py); the one-iteration bound is ``step_bound`` of tests/gstep_cases.py.  No frame is left out of any
comparison.  Every measured error is printed beside its bound."""
import contextlib
import io

import numpy as np
import pytest

from conftest import load_golden
from gstep_cases import EPS, golden, stiff_case
from pdsolve_cases import KS, MODES, NAMES, animate, bound_K, chain, host_case, model
from reduced_forces_cases import bound as rf_bound, case as rf_case, operator as rf_operator
from test_gpu_cforces import _bound as force_bound, _g, _spec
from test_gpu_cproj import RAW_TOL, _kappa, _min_edge
from test_gpu_gstep import _case, _report

pytestmark = pytest.mark.gpu

CHAINS = [2, 15, 16, 17, 31, 32, 33, 65]
MESHES = ["tets_strain", "tris_strain", "stiff"] + ["chain%d" % n for n in CHAINS]
FRAMES = [1, 63, 64, 65, 130]
_meshes = {}


def _snaps(frames, standarize=False, mass=None):
    from animsnapbases_amd import posSnapshots
    with contextlib.redirect_stdout(io.StringIO()):
        return posSnapshots.from_arrays(np.array(frames), None, "first", standarize=standarize, massWeight=mass is not None, mass=mass)


def _mesh(name):
    """(130 frames, kinds, masses, dt) of a golden kind, the stiff box or an edge-spring chain; built once."""
    if name not in _meshes:
        if name == "stiff":
            c = stiff_case()
            _meshes[name] = (animate(c["rest"], 130, seed=5), [dict(kind="tets_strain", elements=c["tets"], wi=c["wi"], rest_positions=c["rest"])],
                             c["masses"], c["dt"])
        elif name.startswith("chain"):
            rest, edges, m = chain(int(name[5:]))
            _meshes[name] = (animate(rest, 130, seed=6), [dict(kind="edge_spring", elements=edges, wi=2.0, rest_positions=rest)], m, 0.25)
        else:
            z, frames, kinds, _ = _case(name)
            _meshes[name] = (frames, kinds, z["masses"], float(z["dt"]))
    return _meshes[name]


# ------------------------------------------------------------------ 1. against the reference's loop
@pytest.mark.parametrize("name", NAMES)
def test_solve_matches_the_reference_loop(name):
    z, frames, kinds, one = _case(name)
    p = load_golden("pdsolve_" + name)
    F, N = frames.shape[:2]
    snaps = _snaps(frames)
    for mode in MODES:
        for K in KS:
            out, nF = snaps.solve_frames(kinds, float(z["dt"]), K, z["masses"], velocity=mode)
            assert nF == F and tuple(out.shape) == (F, N, 3) and str(out.dtype) == "torch.float64" and out.is_cuda
            B = bound_K(one[mode], K, float(p["amp_%s_%d" % (mode, K)]))
            assert _report("%s %s K = %d" % (name, mode, K), out.cpu().numpy(), p["q_%s_%d" % (mode, K)], B) <= B
    assert list(snaps.assembly_ST) == [k["kind"] for k in kinds]


@pytest.mark.parametrize("name", NAMES)
def test_weighted_standardised_tensor_and_heldout(name):
    kind = "tets_strain" if name == "combined" else name
    g = _g(kind)[0]
    if name == "combined":
        tol_p = 64 * EPS * np.abs(g["frames"]).max() * max(_kappa(k, _g(k)[0]) / _min_edge(k, _g(k)[0]) for k in ("edge_spring", "tets_strain"))
    else:
        tol_p = 64 * EPS * np.abs(g["frames"]).max() / _min_edge(kind, g) * _kappa(kind, g)
    z, frames, kinds, one = _case(name, tol_p)
    p = load_golden("pdsolve_" + name)
    N = frames.shape[1]
    mass = 0.5 + np.random.default_rng(3).random(N)                 # the weighting of the tensor is not the solver's mass
    snaps = _snaps(frames, standarize=True, mass=mass)
    assert snaps.pre_scale_factor != 1 and snaps.massL is not None
    held = _snaps(frames[:3], standarize=True, mass=mass)
    for mode in MODES:
        for K in KS:
            B = bound_K(one[mode], K, float(p["amp_%s_%d" % (mode, K)]))
            ref = p["q_%s_%d" % (mode, K)]
            out, _ = snaps.solve_frames(kinds, float(z["dt"]), K, z["masses"], velocity=mode)
            assert _report("%s %s K = %d weighted" % (name, mode, K), out.cpu().numpy(), ref, B) <= B
            # frame 13 of the fixture is frame 3 of the held-out tensor, whose previous frame is the fixture's frame 12
            out, nF = held.solve_frames(kinds, float(z["dt"]), K, z["masses"], velocity=mode, animation=np.array(frames[10:]),
                                        frame_start=3, frame_jump=2, chunk_frames=16)
            assert nF == ref[13::2].shape[0]
            assert _report("%s %s K = %d held-out" % (name, mode, K), out.cpu().numpy(), ref[13::2], B) <= B


# ------------------------------------------------------------------ 2. one iteration from the frame is global_step, bit for bit
@pytest.mark.parametrize("name", MESHES)
def test_one_iteration_from_the_frame_is_global_step(name):
    import torch
    frames, kinds, m, dt = _mesh(name)
    snaps = _snaps(frames)
    for F in FRAMES:
        for mode in MODES:
            step = snaps.global_step(kinds, dt, m, velocity=mode, frame_end=F)[0]
            got, nF = snaps.solve_frames(kinds, dt, 1, m, velocity=mode, start="frame", frame_end=F)
            assert nF == F and torch.isfinite(got).all()
            assert torch.equal(got, step), (name, F, mode)


# ------------------------------------------------------------------ 3. a + b iterations = b iterations started at the result of a
@pytest.mark.parametrize("name", MESHES)
def test_semigroup(name):
    import torch
    frames, kinds, m, dt = _mesh(name)
    snaps = _snaps(frames)
    for F in FRAMES:
        kw = dict(velocity="difference", frame_end=F)
        for a, b in ((1, 1), (2, 3), (9, 1)):
            whole = snaps.solve_frames(kinds, dt, a + b, m, **kw)[0]
            first = snaps.solve_frames(kinds, dt, a, m, **kw)[0]
            # the iterations move (a single spring keeps its direction and is at its fixed point after one iteration)
            assert frames.shape[1] == 2 or not torch.equal(first, whole)
            keep = first.clone()
            assert torch.equal(snaps.solve_frames(kinds, dt, b, m, start=first, **kw)[0], whole), (name, F, a, b)
            assert torch.equal(first, keep)                          # the start tensor is the caller's and stays
    # the padding of the iterate leaves no trace: a short solve after a long one that filled every column of the buffer
    for F in (65, 1):
        want = snaps.solve_frames(kinds, dt, 3, m, frame_end=F)[0]
        snaps.solve_frames(kinds, dt, 2, m, start=torch.full((128, frames.shape[1], 3), 1e30, dtype=torch.float64, device=want.device),
                           frame_end=128)
        assert torch.equal(snaps.solve_frames(kinds, dt, 3, m, frame_end=F)[0], want)
        two = snaps.solve_frames(kinds, dt, 2, m, start=snaps.solve_frames(kinds, dt, 1, m, frame_end=F)[0], frame_end=F)[0]
        assert torch.equal(two, want)


# ------------------------------------------------------------------ 4. repeats, sub-ranges, chunks, stale buffers
@pytest.mark.parametrize("name", ["tets_strain", "tris_strain", "combined"])
def test_repeats_ranges_and_chunks_are_bit_identical(name):
    import torch
    z, frames, kinds, _ = _case(name)
    dt, m = float(z["dt"]), z["masses"]
    snaps = _snaps(frames)
    for mode in MODES:
        full = snaps.solve_frames(kinds, dt, 3, m, velocity=mode)[0]
        assert torch.equal(snaps.solve_frames(kinds, dt, 3, m, velocity=mode)[0], full)
        part, nF = snaps.solve_frames(kinds, dt, 3, m, velocity=mode, frame_start=3, frame_end=67, frame_jump=2)
        assert nF == 32 and torch.equal(part, full[3:67:2])
        assert torch.equal(snaps.solve_frames(kinds, dt, 3, m, velocity=mode, chunk_frames=16)[0], full)


def test_a_solve_after_a_solve_of_another_shape_equals_a_fresh_context():
    import torch
    frames, kinds, m, dt = _mesh("chain33")
    fresh = _snaps(frames[:20]).solve_frames(kinds, dt, 3, m)[0]
    big_frames, big_kinds, big_m, big_dt = _mesh("stiff")
    # one context: first the larger mesh through its own snapshots, then -- on the SAME engine -- the smaller mesh with more frames
    big = _snaps(big_frames[:5])
    big.solve_frames(big_kinds, big_dt, 2, big_m)
    from animsnapbases_amd import posSnapshots
    with contextlib.redirect_stdout(io.StringIO()):
        small = posSnapshots.from_arrays(np.array(frames[:20]), None, "first", standarize=False, massWeight=False, engine=big._engine)
    assert small._engine is big._engine
    assert torch.equal(small.solve_frames(kinds, dt, 3, m)[0], fresh)
    # and on one tensor: a reduced then a full solve, more kinds then fewer, more frames then fewer
    z, fr, both, _ = _case("combined")
    snaps = _snaps(fr)
    want = _snaps(fr).solve_frames(both[1:], float(z["dt"]), 2, z["masses"], frame_end=7)[0]
    snaps.solve_frames(both, float(z["dt"]), 2, z["masses"])
    assert torch.equal(snaps.solve_frames(both[1:], float(z["dt"]), 2, z["masses"], frame_end=7)[0], want)


# ------------------------------------------------------------------ 5. the history of step sizes
@pytest.mark.parametrize("name", ["tets_strain", "tris_strain"])
def test_history_matches_the_step_norms_of_the_iterates(name):
    import torch
    frames, kinds, m, dt = _mesh(name)
    F, N = frames.shape[:2]
    K = 3
    snaps = _snaps(frames)
    q0 = 2.0 * frames - frames[[max(f - 1, 0) for f in range(F)]]
    start = torch.from_numpy(q0).to("cuda:%d" % snaps._engine.device_id)
    out, nF, hist = snaps.solve_frames(kinds, dt, K, m, start=start, history=True)
    assert nF == F and hist.shape == (K, F) and np.isfinite(hist).all()
    assert torch.equal(out, snaps.solve_frames(kinds, dt, K, m, start=start)[0])     # asking for the history changes no bit
    again = snaps.solve_frames(kinds, dt, K, m, start=start, history=True)[2]
    assert np.array_equal(again, hist)
    q = [q0] + [snaps.solve_frames(kinds, dt, k, m, start=start)[0].cpu().numpy() for k in range(1, K + 1)]
    # the device's iterates are within B_K of the exact ones of its own start (q_0 = s, the start of the fixture's amp); the
    # ratio is Lipschitz in both arguments (tests/test_gpu_gstep.py, test 6), each norm a sum of n = 3 N squares in floating point
    one = _case(name)[3]
    B = bound_K(one["difference"], K, max(float(load_golden("pdsolve_" + name)["amp_difference_%d" % k]) for k in KS))
    n = 3 * N
    for k in range(1, K + 1):
        nk = np.linalg.norm(q[k].reshape(F, -1), axis=1)
        r = np.linalg.norm((q[k] - q[k - 1]).reshape(F, -1), axis=1) / nk
        tol = (2 * B + r * B) * np.sqrt(n) / nk * (1.0 + 4 * n * EPS) * 2 + 4 * n * EPS * r
        err = np.abs(hist[k - 1] - r)
        print("%s iteration %d: step %.3g .. %.3g, largest err / tol %.3g" % (name, k, r.min(), r.max(), (err / tol).max()))
        assert (err <= tol).all() and (r > 0).all()


# ------------------------------------------------------------------ 6. a reduced kind
def _reduced_one(c, z, m, q):
    fb = force_bound(_g(c.kind)[2], c.g["expected"], RAW_TOL).max()
    return z["Ainv_abs_inf"] * max(fb, rf_bound(c, m, rf_operator(c, m)).max()) + 64 * EPS * z["kappa"] * np.abs(q).max()


def _reduced_kw(c):
    return dict(elements=c.g["elements"], wi=0.7, rest_positions=c.g["rest"], sigma_min=c.g["sigma"][0], sigma_max=c.g["sigma"][1])


@pytest.mark.parametrize("fixture", ["tets_deim", "tris_blocks"])
def test_reduced_solve_matches_the_host_route(fixture):
    c = rf_case(fixture)
    z = golden(c.kind)
    hc = host_case(c.kind)
    amps = load_golden("pdsolve_reduced_" + fixture)
    frames = c.g["frames"]
    F = frames.shape[0]
    dt, masses = float(z["dt"]), z["masses"]
    snaps = _snaps(frames)
    assert amps["ms"].tolist() == [c.ms[0], c.ms[-1]]
    coarse = None
    for m in (c.ms[0], c.ms[-1]):
        spec = dict(kind=c.kind, basis=c.basis, num_components=m, reduction=c.reduction, **_reduced_kw(c))
        for mode in MODES:
            host = model(hc, range(F), mode, KS, reduced=(0, rf_operator(c, m)))
            coarse = host[10] if coarse is None else coarse         # (smallest m, velocity "zero")
            for K in KS:
                out, nF = snaps.solve_frames([spec], dt, K, masses, velocity=mode)
                B = bound_K(_reduced_one(c, z, m, host[K]), K, float(amps["amp_%d_%s_%d" % (m, mode, K)]))
                assert nF == F and _report("%s m = %d %s K = %d" % (fixture, m, mode, K), out.cpu().numpy(), host[K], B) <= B
    # the reduced term differs from the full one: the comparison above is not vacuous
    full = snaps.solve_frames([dict(kind=c.kind, **_reduced_kw(c))], dt, 10, masses, velocity="zero")[0].cpu().numpy()
    assert np.abs(full - coarse).max() > B


def test_reduced_solve_errors_against_the_host_route():
    from animsnapbases_amd import constraintsComponents as cc
    c = rf_case("tets_deim")
    z = golden("tets_strain")
    hc = host_case("tets_strain")
    amps = load_golden("pdsolve_reduced_tets_deim")
    frames = c.g["frames"]
    F, N = frames.shape[:2]
    dt, masses, K = float(z["dt"]), z["masses"], 3
    kw = dict(reduction=c.reduction, **_reduced_kw(c))
    snaps = _snaps(frames)
    rs = [c.ms[0], c.ms[-1]]
    got = snaps.reduced_solve_errors(c.kind, c.basis, rs, dt, K, masses, per_frame=True, **kw)
    assert got[5].shape == (len(rs), F) and all(len(v) == len(rs) for v in got[:5])
    q = model(hc, range(F), "difference", (K,))[K]
    amp_full = float(load_golden("pdsolve_tets_strain")["amp_difference_%d" % K])
    n = 3 * F * N
    for i, r in enumerate(rs):
        qt = model(hc, range(F), "difference", (K,), reduced=(0, rf_operator(c, r)))[K]
        # each device tensor is within B of the host's; the metrics are Lipschitz in their two arguments
        B = bound_K(_reduced_one(c, z, r, q), K, max(amp_full, float(amps["amp_%d_difference_%d" % (r, K)])))
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
    # one iteration from the frame: exactly the numbers of reduced_global_step_errors
    one = snaps.reduced_solve_errors(c.kind, c.basis, c.ms, dt, 1, masses, start="frame", per_frame=True, **kw)
    old = snaps.reduced_global_step_errors(c.kind, c.basis, c.ms, dt, masses, per_frame=True, **kw)
    assert all(one[j] == old[j] for j in range(5)) and np.array_equal(one[5], old[5])
    # a sweep equals single calls; nothing depends on the order
    single = snaps.reduced_solve_errors(c.kind, c.basis, [rs[1]], dt, K, masses, **kw)
    assert [v[0] for v in single] == [got[j][1] for j in range(5)]
    assert snaps.reduced_solve_errors(c.kind, c.basis, [], dt, K, masses, **kw) == ([], [], [], [], [])


# ------------------------------------------------------------------ 7. NaN containment
def test_collapsed_edge_poisons_exactly_its_frame():
    g, s, _ = _g("edge_spring_collapsed")
    nan_frames = np.isnan(s["b"]).any(axis=(1, 2))
    assert nan_frames.tolist() == [False, False, True, False]
    N = g["rest"].shape[0]
    snaps = _snaps(g["frames"])
    kinds = [_spec("edge_spring_collapsed")]
    # the edge is collapsed in x_2: in the start "frame", and in the explicit state of velocity "zero" (s = x)
    for kw in (dict(start="frame", velocity="zero"), dict(start="frame", velocity="difference"), dict(start="explicit", velocity="zero")):
        out = snaps.solve_frames(kinds, 0.5, 3, np.ones(N), **kw)[0].cpu().numpy()
        assert np.isnan(out[nan_frames]).all() and np.isfinite(out[~nan_frames]).all(), kw


# ------------------------------------------------------------------ 8. refusals at both layers
def test_refusals():
    import torch
    from animsnapbases_amd import _lib
    z, frames, kinds, _ = _case("tets_strain")
    F, N = frames.shape[:2]
    dt, m = float(z["dt"]), z["masses"]
    snaps = _snaps(frames)
    eng = snaps._engine
    dev = "cuda:%d" % eng.device_id
    # no solve begun: the solve's entries refuse, at the C layer
    with pytest.raises(RuntimeError, match="no solve begun"):
        eng.pdsolve_slot(1.0, 1.0, None)
    with pytest.raises(RuntimeError, match="no solve begun"):
        eng.pdsolve_iterate(1)
    with pytest.raises(RuntimeError, match="asb_gstep_setup"):      # no inverse yet
        eng.pdsolve_begin(0, 0, F, 1, None, False, 1.0, np.ones(N), 0, np.zeros(3), 0)
    good = snaps.solve_frames(kinds, dt, 1, m, frame_end=4)[0]
    assert tuple(good.shape) == (4, N, 3)
    for bad in (torch.zeros((4, N, 3), dtype=torch.float32, device=dev), torch.zeros((4, N + 1, 3), dtype=torch.float64, device=dev),
                torch.zeros((4, N), dtype=torch.float64, device=dev), torch.zeros((5, N, 3), dtype=torch.float64, device=dev),
                torch.zeros((4, N, 3), dtype=torch.float64), torch.zeros((4, 3, N), dtype=torch.float64, device=dev).transpose(1, 2),
                np.zeros((4, N, 3))):
        with pytest.raises(ValueError, match="start"):
            snaps.solve_frames(kinds, dt, 1, m, start=bad, frame_end=4)
    with pytest.raises(ValueError, match="num_iterations"):
        snaps.solve_frames(kinds, dt, 0, m)
    with pytest.raises(RuntimeError, match="iterations"):
        eng.pdsolve_iterate(0)
    c = rf_case("tets_deim")
    red = dict(kind=c.kind, basis=c.basis, num_components=c.ms[0], reduction=c.reduction, elements=c.g["elements"], wi=0.7,
               rest_positions=c.g["rest"], sigma_min=c.g["sigma"][0], sigma_max=c.g["sigma"][1])
    with pytest.raises(ValueError, match="second reduced kind"):
        snaps.solve_frames([red, dict(red, kind="tets_deformation_gradient")], dt, 1, m)
    # ... and at the C layer: a solve with one reduced slot refuses another
    snaps.solve_frames([red], dt, 1, m, frame_end=4)
    from animsnapbases_amd import projections as proj
    eng.cproj_setup(proj.subset_setup(proj.build_setup(c.kind, c.g["elements"], c.g["rest"]), rf_operator(c, c.ms[0]).elements))
    with pytest.raises(RuntimeError, match="second reduced kind"):
        eng.pdsolve_slot(1.0, 1.0, None)
    # a slot without an element set-up; a begun solve without a kind
    eng.pdsolve_begin(0, 0, 4, 1, None, False, 1.0, m / dt ** 2, 1, np.zeros(3), 0)
    with pytest.raises(RuntimeError, match="no kind registered"):
        eng.pdsolve_iterate(1)
    # more frames than the grid limit, at the C entry: the count alone is refused, nothing behind the pointers is read
    one = np.ones(1)
    rc = eng.lib.asb_pdsolve_begin(eng.h, 0, 0, 65535 * 64 + 1, 1, None, 0, 1.0, _lib.ptr(one), 0, _lib.ptr(one), 0, None)
    assert rc == _lib.ERR_LIMIT and b"4194240" in eng.lib.asb_last_error(eng.h)
    with pytest.raises(RuntimeError, match="no solve begun"):       # the refused begin left no solve behind
        eng.pdsolve_iterate(1)
    with pytest.raises(ValueError, match="velocity"):
        snaps.solve_frames(kinds, dt, 1, m, velocity="leapfrog")
    with pytest.raises(ValueError, match="empty frame range"):
        snaps.solve_frames(kinds, dt, 1, m, frame_start=F)
    assert torch.equal(snaps.solve_frames(kinds, dt, 1, m, frame_end=4)[0], good)      # and the object still works
