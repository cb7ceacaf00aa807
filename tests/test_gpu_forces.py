"""GPU (-m gpu): external forces and the floor in the resident time steps -- asb_ext_set / asb_pdsolve_external and the fused pass of
asb_pdsolve_advance (csrc/asb_pdsolve.hip), and ``forces=`` / ``floor=`` of posSnapshots.simulate_frames / solve_frames /
reduced_rollout_errors -- against the fixtures of the UNMODIFIED reference's ``step()`` with a force per step and
its ``resolve_collision`` (tools/gen_golden_forces.py), step by step against one NumPy step from the device's OWN two previous
records, bit for bit against itself, and at the C entries' refusals.

Shapes.  The kernels' block is 64 rows x 64 frames of the (3 N, F') state: chains of N in {2, 21, 22, 65} (3 N = 63 and 66 straddle the
row tile, 195 = three tiles and a ragged one) at F' in {1, 63, 64, 65, 130} with frame_jump in {1, 3} (the table row differs per lane),
a constant table, one row per step, the ``vertices`` form, force only, floor only, the floor along each axis; and the goldens
(N = 18, 42; F' = 44).

Bounds: tests/forces_cases.py -- B of rollout_cases with the carry's rounding extended by the one of the add; amp measured on the
host model and stored with the fixtures.  No start frame is left out.  Every error is printed beside its bound."""
import contextlib
import io

import numpy as np
import pytest
from scipy import sparse
from scipy.sparse.linalg import splu

import forces_cases as fc
from conftest import load_golden
from gstep_cases import EPS, golden
from pdsolve_cases import KS, MODES, animate, chain
from reduced_forces_cases import case as rf_case
from rollout_cases import START_FRAMES, iterate
from test_gpu_cforces import _g
from test_gpu_cproj import RAW_TOL, _kappa, _min_edge
from test_gpu_gstep import _case, _report
from test_gpu_pdsolve import _mesh, _reduced_kw, _snaps
from test_gpu_rollout import G as G_CHAIN, _chain_bound, _dev, _prev

pytestmark = pytest.mark.gpu

CHAINS = [2, 21, 22, 65]
FRAMES = [1, 63, 64, 65, 130]
JUMPS = [1, 3]
SEL = dict(frame_jump=3)                                            # range(0, 130, 3): START_FRAMES


# ------------------------------------------------------------------ 1. against the reference's steps with its force and floor
def _against_reference(name, snaps, tol_p, tag):
    import torch
    z = load_golden("forces_" + name)
    zg, frames, kinds, one = _case(name, tol_p)
    dt, masses = float(zg["dt"]), zg["masses"]
    forces = dict(force=z["force"])
    floor = dict(height=float(z["floor"]), axis=1) if "floor" in z else None
    assert (floor is not None) == fc.FIXTURES[name]
    acc = dt * dt * np.array(fc.G)
    fa = fc.fa_of(z["force"], masses, dt)
    steps = z["steps"].tolist()
    T = max(steps)
    kw = dict(gravity=fc.G, **SEL)
    worst = 0.0
    for mode in MODES:
        for K in KS:
            q, q_prev, nF, (rec, rsteps) = snaps.simulate_frames(kinds, dt, T, K, masses, velocity=mode, record_every=1, forces=forces,
                                                                 floor=floor, **kw)
            assert nF == len(START_FRAMES) and rsteps == list(range(1, T + 1))
            got = rec.cpu().numpy()
            loose = snaps.simulate_frames(kinds, dt, T, K, masses, velocity=mode, record_every=1, **kw)[3][0].cpu().numpy()
            for t in steps:
                ref = z["q_%s_%d_%d" % (mode, K, t)]
                B = fc.bound_T(one[mode], K, t, float(z["amp_%s_%d_%d" % (mode, K, t)]), ref, acc, fa)
                err = _report("%s %s K = %d T = %d %s" % (name, mode, K, t, tag), got[t - 1], ref, B)
                assert err <= B
                worst = max(worst, err / B)
                assert np.abs(loose[t - 1] - got[t - 1]).max() > B     # the force and the floor matter
            # the fixture's first step is solve_frames with the same keywords
            out = snaps.solve_frames(kinds, dt, K, masses, velocity=mode, forces=forces, floor=floor, **kw)[0]
            assert torch.equal(out, rec[0])
    print("%s %s: largest err / B %.3g" % (name, tag, worst))


@pytest.mark.parametrize("name", sorted(fc.FIXTURES))
def test_steps_with_forces_and_floor_match_the_reference(name):
    _against_reference(name, _snaps(_case(name)[1]), RAW_TOL, "raw")


@pytest.mark.parametrize("name", sorted(fc.FIXTURES))
def test_steps_with_forces_and_floor_on_a_weighted_standardised_tensor(name):
    g = _g(name)[0]
    tol_p = 64 * EPS * np.abs(g["frames"]).max() / _min_edge(name, g) * _kappa(name, g)
    mass = 0.5 + np.random.default_rng(3).random(g["frames"].shape[1])         # the weighting of the tensor is not the solver's mass
    snaps = _snaps(g["frames"], standarize=True, mass=mass)
    assert snaps.pre_scale_factor != 1 and snaps.massL is not None
    _against_reference(name, snaps, tol_p, "weighted")


# ------------------------------------------------------------------ 2. chains: every step against one host step of the device's own records
_chains = {}
N_FRAMES = 3 * 129 + 2                                              # frame_jump 3 at F' = 130 reads frame 387


def _long_chain(n):
    """The chain of ``pdsolve_cases.chain`` with an animation long enough for frame_jump 3, as a case of the host model."""
    if n not in _chains:
        from animsnapbases_amd import projections as proj
        rest, edges, m = chain(n)
        frames = animate(rest, N_FRAMES, seed=6)
        dt, wi = 0.25, 2.0
        setup = proj.build_setup("edge_spring", edges, rest)
        St = proj.assembly_ST(setup, n, wi)
        A = proj.global_matrix([(setup, wi)], n, m, dt)
        Ad = A.toarray()
        _chains[n] = dict(frames=frames, kinds=[(setup, St, 1.0, 1.0)], masses=m, dt=dt, lu=splu(sparse.csc_matrix(A)),
                          spec=[dict(kind="edge_spring", elements=edges, wi=wi, rest_positions=rest)],
                          Ainv_abs_inf=np.abs(np.linalg.inv(Ad)).sum(axis=1).max(), kappa=np.linalg.cond(Ad),
                          d=np.linalg.norm(rest[edges[:, 1]] - rest[edges[:, 0]], axis=1), edges=edges, snaps=_snaps(frames))
    return _chains[n]


def _variant(i, n, frames):
    """(forces dict or None, fa as the host model reads it or None, floor dict or None) number i: the table's forms and the
    floor's axes in turn, force only and floor only among them."""
    rng = np.random.default_rng(50 + i)
    rows = N_FRAMES + 8
    form = i % 4
    forces = dense = None
    if i % 7 != 6:
        if form == 0:                                               # a constant force
            dense = 5.0 * rng.standard_normal((n, 3))
            forces = dict(force=dense)
        elif form == 1:                                             # one row per step
            dense = 5.0 * rng.standard_normal((rows, n, 3))
            forces = dict(force=dense, start=2)
        else:                                                       # the vertices form, per step (2) or constant (3)
            v = rng.permutation(n)[:max(1, n // 2)]
            f = 5.0 * rng.standard_normal(((rows,) if form == 2 else ()) + (v.size, 3))
            dense = np.zeros(f.shape[:-2] + (n, 3))
            dense[..., v, :] = f
            forces = dict(force=f, vertices=v, start=2 if form == 2 else 0)
    floor = None
    if forces is None or i % 5 != 4:
        axis = i % 3
        floor = dict(height=float(np.quantile(frames[..., axis], 0.4)), axis=axis)
    return forces, dense, floor


@pytest.mark.parametrize("n", CHAINS)
def test_every_step_is_one_host_step_from_the_devices_own_records(n):
    c = _long_chain(n)
    frames, dt, snaps = c["frames"], c["dt"], c["snaps"]
    acc = dt * dt * np.array(G_CHAIN)
    diag = (c["masses"] / dt ** 2).max()
    T, i = 4, 0
    for F in FRAMES:
        for fj in JUMPS:
            forces, dense, floor = _variant(i + n, n, frames)
            mode = MODES[i % 2]
            i += 1
            sel = list(range(0, (F - 1) * fj + 1, fj))
            kw = dict(velocity=mode, gravity=G_CHAIN, frame_end=sel[-1] + 1, frame_jump=fj)
            q, q_prev, nF, (rec, steps) = snaps.simulate_frames(c["spec"], dt, T, 1, c["masses"], record_every=1, forces=forces, floor=floor, **kw)
            assert nF == F and steps == [1, 2, 3, 4]
            r = rec.cpu().numpy()
            assert np.isfinite(r).all()
            fa = None if dense is None else fc.fa_of(dense, c["masses"], dt)
            rows = np.array(sel) + (0 if forces is None else forces.get("start", 0))
            fl = None if floor is None else (floor["height"], floor["axis"])
            x0 = frames[sel]
            hist = [x0 if mode == "zero" else _prev(frames, sel), x0] + list(r)
            worst = 0.0
            for t in range(1, T + 1):
                s = 2.0 * hist[t] - hist[t - 1] + acc[None, None, :]
                x, hit = fc.external(s, fc.rows_of(fa, rows + t - 1), fl)
                want = iterate(c, x, x, 1)
                B = _chain_bound(c, x, want) + c["Ainv_abs_inf"] * diag * fc.ext_bound(s, fa)
                err = np.abs(r[t - 1] - want).max()
                worst = max(worst, err / B)
                assert err <= B, (n, F, fj, forces is None, floor, mode, t, err, B)
            # the next row of the table, or no force and no floor at all, is further away than the bound
            if fa is not None and fa.ndim == 3:
                other = iterate(c, *(2 * (fc.external(s, fc.rows_of(fa, rows + T), fl)[0],)), 1)
                assert np.abs(r[T - 1] - other).max() > B
            loose = snaps.simulate_frames(c["spec"], dt, T, 1, c["masses"], **kw)[0].cpu().numpy()
            assert np.abs(loose - r[T - 1]).max() > B
            print("chain %d F' = %d jump %d %s force %s floor %s: largest err / bound %.3g (bound %.3g)"
                  % (n, F, fj, mode, None if dense is None else dense.shape, fl, worst, B))


def test_the_chains_cover_every_form_and_axis():
    """What the parametrised test above runs, counted without the device: every table form, force only, floor only, each axis."""
    seen = set()
    for n in CHAINS:
        for i in range(len(FRAMES) * len(JUMPS)):
            forces, dense, floor = _variant(i + n, n, np.zeros((2, n, 3)))
            seen.add((None if forces is None else (dense.ndim, "vertices" in forces), None if floor is None else floor["axis"]))
    forms = {s[0] for s in seen}
    assert forms == {None, (2, False), (3, False), (2, True), (3, True)}
    assert {s[1] for s in seen} == {None, 0, 1, 2} and all(f is not None or a is not None for f, a in seen)


# ------------------------------------------------------------------ 3. bit identities
def _table(N, rows=140, seed=0):
    return 3.0 * np.random.default_rng(90 + N + seed).standard_normal((rows, N, 3))


@pytest.mark.parametrize("name", ["chain21", "chain22", "chain65", "tris_strain"])
def test_paths_with_forces_and_floor_are_bit_identical(name):
    import torch
    frames, kinds, m, dt = _mesh(name)
    N = frames.shape[1]
    snaps = _snaps(frames)
    G = (0.0, -1.0, 0.3)
    force = _table(N)
    floor = dict(height=float(np.quantile(frames[..., 1], 0.5)), axis=1)
    forces = dict(force=force, start=1)
    for F in FRAMES:
        kw = dict(gravity=G, frame_end=F)
        ext = dict(forces=forces, floor=floor)
        for mode in MODES:
            # one step of a roll-out is solve_frames from the explicit state
            q, q_prev, nF = snaps.simulate_frames(kinds, dt, 1, 3, m, velocity=mode, **ext, **kw)
            assert nF == F and torch.equal(q, snaps.solve_frames(kinds, dt, 3, m, velocity=mode, start="explicit", **ext, **kw)[0])
            assert not torch.equal(q, snaps.simulate_frames(kinds, dt, 1, 3, m, velocity=mode, **kw)[0])
            # a solve continued from its own result is the longer solve: the inertia term is formed without touching the iterate
            a = snaps.solve_frames(kinds, dt, 1, m, velocity=mode, **ext, **kw)[0]
            assert torch.equal(snaps.solve_frames(kinds, dt, 2, m, velocity=mode, start=a, **ext, **kw)[0], q)
            # from the frame: the same inertia term under another first iterate
            fr = snaps.solve_frames(kinds, dt, 2, m, velocity=mode, start="frame", **ext, **kw)[0]
            X = _dev(snaps, frames[:F])
            assert torch.equal(fr, snaps.solve_frames(kinds, dt, 2, m, velocity=mode, start=X, **ext, **kw)[0]) and not torch.equal(fr, q)
        want = snaps.simulate_frames(kinds, dt, 3, 2, m, record_every=1, **ext, **kw)
        # T1 steps continued by T2 with start raised by T1 are T1 + T2 steps
        for a, b in ((1, 2), (2, 1)):
            q1, p1, _ = snaps.simulate_frames(kinds, dt, a, 2, m, **ext, **kw)
            later = dict(forces=dict(forces, start=forces["start"] + a), floor=floor)
            q2, p2, _ = snaps.simulate_frames(kinds, dt, b, 2, m, state=(q1, p1), **later, **kw)
            assert torch.equal(q2, want[0]) and torch.equal(p2, want[1]) and torch.equal(q1, want[3][0][a - 1])
            assert not torch.equal(snaps.simulate_frames(kinds, dt, b, 2, m, state=(q1, p1), **ext, **kw)[0], want[0])      # (not raised)
        # repeats, a chunk width and a frame sub-range (the rows follow the frames) change no bit
        assert torch.equal(snaps.simulate_frames(kinds, dt, 3, 2, m, record_every=1, **ext, **kw)[3][0], want[3][0])
        assert torch.equal(snaps.simulate_frames(kinds, dt, 3, 2, m, record_every=1, chunk_frames=16, **ext, **kw)[3][0], want[3][0])
        if F > 3:
            part = snaps.simulate_frames(kinds, dt, 3, 2, m, gravity=G, frame_start=1, frame_end=F, frame_jump=2, record_every=1, **ext)
            assert part[2] == len(range(1, F, 2)) and torch.equal(part[3][0], want[3][0][:, 1:F:2]) and torch.equal(part[1], want[1][1:F:2])
        # the vertices form is the same force dense; a constant table is its row repeated
        v = np.array([N - 1, 0, N // 2])
        dense = np.zeros_like(force)
        dense[:, v] = force[:, :3]
        a = snaps.simulate_frames(kinds, dt, 3, 2, m, forces=dict(force=force[:, :3], vertices=v, start=1), floor=floor, **kw)
        b = snaps.simulate_frames(kinds, dt, 3, 2, m, forces=dict(force=dense, start=1), floor=floor, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], want[0])
        a = snaps.simulate_frames(kinds, dt, 3, 2, m, forces=dict(force=force[5]), **kw)
        b = snaps.simulate_frames(kinds, dt, 3, 2, m, forces=dict(force=np.repeat(force[5][None], 140, axis=0), start=4), **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        # a zero table and a floor below every coordinate are the call without the keywords
        bare = snaps.simulate_frames(kinds, dt, 3, 2, m, **kw)
        for low in (dict(forces=dict(force=np.zeros((140, N, 3))), floor=dict(height=-1e6, axis=1)), dict(forces=dict(force=np.zeros((N, 3)))),
                    dict(floor=dict(height=-1e6, axis=0))):
            got = snaps.simulate_frames(kinds, dt, 3, 2, m, **low, **kw)
            assert torch.equal(got[0], bare[0]) and torch.equal(got[1], bare[1])
        assert not torch.equal(bare[0], want[0])
        # the padding columns of Q and P are never written
        snaps.simulate_frames(kinds, dt, 3, 2, m, **ext, **kw)
        ld = (F + 63) // 64 * 64
        for which in (0, 1):
            st = snaps._engine.pdsolve_state(which)
            assert st.shape == (3 * N, ld) and np.all(st[:, F:] == 0.0) and np.isfinite(st[:, :F]).all()
        assert np.array_equal(snaps._engine.pdsolve_state(0)[:, :F].T.reshape(F, -1, 3), want[0].cpu().numpy())


@pytest.mark.parametrize("fixture", ["tris_blocks"])
def test_reduced_and_hyper_paths_with_forces_and_floor_continue_bit_identically(fixture):
    import torch
    c = rf_case(fixture)
    z = golden(c.kind)
    frames = c.g["frames"]
    N = frames.shape[1]
    dt, masses = float(z["dt"]), z["masses"]
    snaps = _snaps(frames)
    spec = [dict(kind=c.kind, basis=c.basis, num_components=c.ms[-1], reduction=c.reduction, **_reduced_kw(c))]
    floor = dict(height=float(np.quantile(frames[..., 1], 0.4)), axis=1)
    force = 0.2 * _table(N)
    whole = {}
    for hyper in (None, "touched", "all"):
        kw = dict(gravity=fc.G, hyper=hyper, floor=floor)
        whole[hyper] = snaps.simulate_frames(spec, dt, 4, 3, masses, record_every=1, forces=dict(force=force, start=2), **kw)
        q1, p1, _ = snaps.simulate_frames(spec, dt, 3, 3, masses, forces=dict(force=force, start=2), **kw)
        q2, p2, _ = snaps.simulate_frames(spec, dt, 1, 3, masses, state=(q1, p1), forces=dict(force=force, start=5), **kw)
        assert torch.equal(q2, whole[hyper][0]) and torch.equal(p2, whole[hyper][1]) and torch.equal(p2, q1)
        assert torch.equal(snaps.simulate_frames(spec, dt, 4, 3, masses, chunk_frames=16, record_every=1, forces=dict(force=force, start=2), **kw)[3][0],
                           whole[hyper][3][0])
        loose = snaps.simulate_frames(spec, dt, 4, 3, masses, gravity=fc.G, hyper=hyper)
        assert not torch.equal(loose[0], whole[hyper][0])
    assert torch.equal(whole["touched"][3][0], whole["all"][3][0]) and torch.equal(whole["touched"][1], whole["all"][1])
    # the hyper-reduced constant c = A^-1 ms picks the force and the floor up: near the plain reduced path, far from the run without them
    a, b = whole[None][3][0].cpu().numpy(), whole["touched"][3][0].cpu().numpy()
    far = np.abs(loose[0].cpu().numpy() - b[-1]).max()
    print("%s: |hyper - reduced| %.3g, |without forces - hyper| %.3g" % (fixture, np.abs(a - b).max(), far))
    assert np.abs(a - b).max() < 1e-6 * far


def test_a_nan_frame_of_the_state_stays_in_its_frame_with_the_floor_on():
    frames, kinds, m, dt = _mesh("chain33")
    snaps = _snaps(frames)
    N = frames.shape[1]
    ext = dict(forces=dict(force=_table(N)), floor=dict(height=float(np.quantile(frames[..., 1], 0.5)), axis=1))
    for F, bad in ((65, 64), (130, 63)):
        for poisoned in (0, 1):
            state = [_dev(snaps, frames[:F]), _dev(snaps, _prev(frames, range(F)))]
            state[poisoned][bad, 5, 1] = float("nan")
            q, p, _, (rec, _) = snaps.simulate_frames(kinds, dt, 4, 2, m, state=tuple(state), record_every=1, gravity=fc.G, frame_end=F, **ext)
            r = rec.cpu().numpy()
            nan = np.isnan(r).any(axis=(2, 3))
            assert nan[:, bad].all() and not np.delete(nan, bad, axis=1).any(), (F, poisoned)


# ------------------------------------------------------------------ 5. refusals of the engine
def test_engine_refusals_return_their_code_and_launch_nothing():
    import torch
    from animsnapbases_amd import _lib
    frames, kinds, m, dt = _mesh("chain17")
    F, N = 5, frames.shape[1]
    snaps = _snaps(frames)
    eng = snaps._engine
    err = lambda: eng.lib.asb_last_error(eng.h)
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    begin = lambda: eng.pdsolve_begin(0, 0, F, 1, None, False, 1.0, m / dt ** 2, 1, np.zeros(3), 0)
    # before any solve, and with nothing set
    eng.ext_set(np.zeros((7, 3 * N)), (0.0, 1))
    assert eng.lib.asb_pdsolve_external(eng.h, 0) == _lib.ERR_ARG and b"no solve begun" in err()
    eng.ext_clear()
    snaps.global_solve_setup(kinds, dt, m)
    begin()
    assert eng.lib.asb_pdsolve_external(eng.h, 0) == _lib.ERR_ARG and b"no forces and no floor" in err()
    # what asb_ext_set refuses leaves nothing set
    ok = f64(np.zeros((7, 3 * N)))
    bad = [(7, None, 0, 1, 0.0, b"missing"), (-1, ok, 0, 1, 0.0, b"rows"), (0, None, 0, 1, 0.0, b"neither"),
           (7, f64(np.full((7, 3 * N), np.nan)), 0, 1, 0.0, b"not finite"), (0, f64(np.full(3 * N, np.inf)), 0, 1, 0.0, b"not finite"),
           (7, ok, 1, 3, 0.0, b"axis"), (7, ok, 1, -1, 0.0, b"axis"), (0, None, 1, 1, float("nan"), b"height"), (0, None, 1, 1, float("inf"), b"height")]
    for T_s, t, on, axis, h, msg in bad:
        assert eng.lib.asb_ext_set(eng.h, T_s, _lib.ptr(t), on, axis, h) == _lib.ERR_ARG and msg in err(), msg
        assert eng.lib.asb_pdsolve_external(eng.h, 0) == _lib.ERR_ARG and b"no forces and no floor" in err()
    # a table of rows 0 .. 6; frames 0 .. 4 read rows 2 .. 6 with row0 = 2
    eng.ext_set(ok, (0.0, 1))
    before = eng.pdsolve_state(0)
    assert eng.lib.asb_pdsolve_external(eng.h, 3) == _lib.ERR_ARG and b"row 7 of the force table" in err()
    assert eng.lib.asb_pdsolve_external(eng.h, -1) == _lib.ERR_ARG
    assert np.array_equal(eng.pdsolve_state(0), before)
    eng.pdsolve_external(2)
    assert eng.lib.asb_pdsolve_external(eng.h, 2) == _lib.ERR_ARG and b"already" in err()
    eng.pdsolve_carry(None)
    before = eng.pdsolve_state(0)
    assert eng.lib.asb_pdsolve_advance(eng.h) == _lib.ERR_ARG and b"row 7 of the force table" in err()     # the next step's row is missing
    assert np.array_equal(eng.pdsolve_state(0), before) and np.array_equal(eng.pdsolve_state(1)[:, :F].T.reshape(F, N, 3), frames[:F])
    # external after the pins is refused: their term would be lost
    rec = snaps._pins("test", dict(vertices=np.array([0, N - 1]), wi=np.array([1.0, 2.0])))
    eng.pins_set(rec.vertices, rec.wi, rec.p0, None)
    begin()
    eng.pdsolve_pins(0)
    before = eng.pdsolve_state(0)
    assert eng.lib.asb_pdsolve_external(eng.h, 0) == _lib.ERR_ARG and b"pins already" in err()
    assert np.array_equal(eng.pdsolve_state(0), before)
    # a begin drops the binding: the advance is the plain one again; clearing drops it too
    begin()
    eng.pdsolve_carry(None)
    eng.pdsolve_advance()
    eng.pdsolve_external(0)
    eng.ext_clear()
    for _ in range(8):
        eng.pdsolve_advance()                                       # (still bound, the third of them would miss its row)
    # a table checked against another N is refused
    eng.ext_set(ok, None)
    from animsnapbases_amd import posSnapshots
    with contextlib.redirect_stdout(io.StringIO()):
        wide = posSnapshots.from_arrays(np.array(_mesh("chain33")[0]), None, "first", standarize=False, massWeight=False, engine=eng)
    wide.global_solve_setup(_mesh("chain33")[1], _mesh("chain33")[3], _mesh("chain33")[2])
    eng.pdsolve_begin(0, 0, F, 1, None, False, 1.0, _mesh("chain33")[2] / _mesh("chain33")[3] ** 2, 1, np.zeros(3), 0)
    assert eng.lib.asb_pdsolve_external(eng.h, 0) == _lib.ERR_ARG and b"checked against" in err()
    del wide
    torch.cuda.synchronize()
    # the public layer refuses a missing row before the engine, and the object still works
    snaps = _snaps(frames)
    with pytest.raises(ValueError, match="row 7 of force is needed"):
        snaps.simulate_frames(kinds, dt, 3, 2, m, frame_end=F, forces=dict(force=np.zeros((7, N, 3)), start=1))
    good = snaps.simulate_frames(kinds, dt, 3, 2, m, frame_end=F, forces=dict(force=np.zeros((7, N, 3))))
    assert torch.equal(good[0], snaps.simulate_frames(kinds, dt, 3, 2, m, frame_end=F)[0])


# ------------------------------------------------------------------ 6. reduced_rollout_errors
def test_reduced_rollout_errors_with_forces_and_floor():
    c = rf_case("tris_blocks")
    z = golden(c.kind)
    frames = c.g["frames"]
    dt, masses = float(z["dt"]), z["masses"]
    kw = dict(reduction=c.reduction, frame_jump=3, gravity=fc.G, **_reduced_kw(c))
    snaps = _snaps(frames)
    rs = [1, c.ms[0], c.ms[-1]]
    ext = dict(forces=dict(force=0.2 * _table(frames.shape[1])), floor=dict(height=float(np.quantile(frames[..., 1], 0.4)), axis=1))
    for hyper in (None, "touched"):
        got = snaps.reduced_rollout_errors(c.kind, c.basis, rs, dt, 4, 3, masses, record_every=2, hyper=hyper, **ext, **kw)
        assert got[5] == [2, 4] and all(a.shape == (len(rs), 2) and np.isfinite(a).all() for a in got[:5])
        for i, r in enumerate(rs):                                  # a sweep equals single calls
            single = snaps.reduced_rollout_errors(c.kind, c.basis, [r], dt, 4, 3, masses, record_every=2, hyper=hyper, **ext, **kw)
            assert all(np.array_equal(single[j][0], got[j][i]) for j in range(5))
        bare = snaps.reduced_rollout_errors(c.kind, c.basis, rs, dt, 4, 3, masses, record_every=2, hyper=hyper, **kw)
        assert not np.array_equal(bare[0], got[0])
        # one step without the keywords reproduces today's numbers
        one = snaps.reduced_rollout_errors(c.kind, c.basis, rs, dt, 1, 3, masses, record_every=1, hyper=hyper, **kw)
        old = snaps.reduced_solve_errors(c.kind, c.basis, rs, dt, 3, masses, hyper=hyper, **kw)
        assert one[5] == [1] and all(one[j][:, 0].tolist() == old[j] for j in range(5))


# ------------------------------------------------------------------ 4. simulate_subspace(forces=): the state in z
def _z_bounds(zm, recs, K, amp, conds, start):
    """``zroll_cases.bounds`` with the force's share of a step (``forces_cases.z_force_bound``) beside the carry's."""
    import rollout_cases as rc
    import zroll_cases as zc
    out, one, adv = [], 0.0, 0.0
    for t, rec in enumerate(recs):
        one, adv = max(one, zc.one_bound(zm, rec, conds)), max(adv, zc.adv_bound(zm, rec) + fc.z_force_bound(zm, rec))
        a = float(amp[t])
        out.append(rc.bound_T(one, K, t + 1, a, adv) + 2.0 * max(1.0, a) * start)
    return out


@pytest.mark.parametrize("fixture,r,m,K,T", [("tris_blocks", 4, 8, 3, 5), ("tris_blocks", 8, 3, 1, 5), ("tets_deim", 4, 17, 3, 5)])
def test_z_rollouts_with_forces_match_the_host_model(fixture, r, m, K, T):
    import zroll_cases as zc
    from test_gpu_gsub import _fixture_snaps
    from test_gpu_hyper import _spec as hyper_spec
    from test_gpu_zroll import _expand_bound, _unorm
    s = zc.z_case(fixture, r)
    op = zc.operator(s, m)
    frames = np.array(s["frames"])
    N = frames.shape[1]
    acc = s["dt"] ** 2 * np.array(fc.G)
    force = fc.force_of(N)
    snaps = _fixture_snaps(frames, r)
    kinds = [hyper_spec(s["rf"], m)]
    x = frames[zc.SEL]
    worst = 0.0
    for mode, table, start in (("zero", force, 1), ("difference", force[3], 0)):      # one row per step; a constant force
        fa = fc.fa_of(table, s["masses"], s["dt"])
        zm = fc.z_model(s, {0: op}, acc, fa)
        amp = fc.measure_amp(dict(s, frames=s["proj_frames"]), mode, K, T, zc.SEL, acc, fa, None, reduced=(0, op))
        kw = dict(velocity=mode, gravity=fc.G, record_every=1, frame_jump=3)
        z, zp, nF, (rec, steps) = snaps.simulate_subspace(kinds, s["dt"], T, K, s["masses"], forces=dict(force=table, start=start), **kw)
        assert nF == len(zc.SEL) and steps == list(range(1, T + 1))
        zs, recs = zm.rollout(*zm.start(frames, zc.SEL, mode), K, T, None, np.array(zc.SEL) + start)
        B = _z_bounds(zm, recs, K, amp, zc.conds_of({0: op}), 3 * zc.start_bound(zm, x))
        got = rec.cpu().numpy()
        un = _unorm(zm)
        for t in range(T):
            ez = float(np.abs(got[t] - zs[t]).max())
            q = snaps.subspace_expand(rec[t]).cpu().numpy()
            eq = float(np.abs(q - zm.expand(zs[t])).max())
            Bq = B[t] + float(_expand_bound(zm, got[t]).max())
            print("%s r = %d m = %d K = %d %s step %d: |dz| %.3g (bound %.3g), |dq| %.3g (bound %.3g), err / bound %.3g"
                  % (fixture, r, m, K, mode, t + 1, ez, un * B[t], eq, Bq, max(ez / (un * B[t]), eq / Bq)))
            assert ez <= un * B[t] and eq <= Bq
            worst = max(worst, ez / (un * B[t]), eq / Bq)
        # without the force, and with the table read one row further, the roll-out is somewhere else by more than the bound
        loose = snaps.subspace_expand(snaps.simulate_subspace(kinds, s["dt"], T, K, s["masses"], **kw)[0]).cpu().numpy()
        assert np.abs(loose - q).max() > Bq
        if table.ndim == 3:
            other = snaps.simulate_subspace(kinds, s["dt"], T, K, s["masses"], forces=dict(force=table, start=start + 1), **kw)[0]
            assert np.abs(snaps.subspace_expand(other).cpu().numpy() - q).max() > Bq
    print("z roll-outs with forces %s r = %d m = %d K = %d T = %d: largest err / bound %.3g" % (fixture, r, m, K, T, worst))


@pytest.mark.parametrize("fixture", ["tets_deim", "tris_blocks"])
def test_z_rollout_with_forces_and_the_full_basis_is_the_hyper_rollout_under_the_inverse(fixture):
    """r = N: the Galerkin step is A^-1, so ``simulate_subspace(forces=)`` is ``simulate_frames(hyper="touched", forces=)`` under
    "inverse"; each lies within its own bound of the exact roll-out, as tests/test_gpu_zroll.py argues without forces."""
    import hyper_cases as hc
    import pdsolve_cases as pc
    import rollout_cases as rc
    import zroll_cases as zc
    from test_gpu_gsub import _fb, _fixture_snaps, _snaps as gsub_snaps
    from test_gpu_hyper import _spec as hyper_spec
    from test_gpu_zroll import _expand_bound
    K, T = 3, 2
    s = zc.z_case(fixture, None)
    c = s["rf"]
    m = c.ms[-1]
    op = zc.operator(s, m)
    full = pc.host_case(c.kind)
    dc = hc.of_host_case(full)
    frames = np.array(s["frames"])
    acc = s["dt"] ** 2 * np.array(fc.G)
    force = fc.force_of(frames.shape[1])
    fa = fc.fa_of(force, s["masses"], s["dt"])
    zm = fc.z_model(s, {0: op}, acc, fa)
    snaps, inv = _fixture_snaps(frames, None), gsub_snaps(frames)
    spec = [hyper_spec(c, m)]
    rows = np.array(zc.SEL) + 2
    for mode in zc.MODES:
        amp = fc.measure_amp(full, mode, K, T, zc.SEL, acc, fa, None, reduced=(0, op))
        zs, recs = zm.rollout(*zm.start(frames, zc.SEL, mode), K, T, None, rows)
        mine = _z_bounds(zm, recs, K, amp, zc.conds_of({0: op}), 3 * zc.start_bound(zm, frames[zc.SEL]))[-1]
        sq, sp = rc.start_state(full["frames"], zc.SEL, mode, acc)
        host = fc.rollout(full, K, T, sq, sp, rows, acc, fa, None, reduced=(0, op))
        one = hc.one_bound(dc["Ainv_abs_inf"], dc["kappa"], c.St, op, c.p_pt(m), np.zeros(3), _fb(c.kind), zc.RAW_TOL, np.abs(host[1]).max())
        theirs = fc.bound_T(one, K, T, float(amp[-1]), host[1], acc, fa)
        kw = dict(velocity=mode, gravity=fc.G, frame_jump=3, forces=dict(force=force, start=2))
        z = snaps.simulate_subspace(spec, s["dt"], T, K, s["masses"], **kw)[0]
        q = snaps.subspace_expand(z).cpu().numpy()
        other = inv.simulate_frames(spec, s["dt"], T, K, s["masses"], hyper="touched", **kw)[0].cpu().numpy()
        both = mine + float(_expand_bound(zm, z.cpu().numpy()).max()) + theirs
        err = float(np.abs(q - other).max())
        print("%s %s r = N with forces: |z roll-out - hyper roll-out under inverse| %.3g, bound %.3g + %.3g, err / bound %.3g"
              % (fixture, mode, err, mine, theirs, err / both))
        assert err <= both
        bare = inv.simulate_frames(spec, s["dt"], T, K, s["masses"], hyper="touched", velocity=mode, gravity=fc.G, frame_jump=3)[0].cpu().numpy()
        assert np.abs(bare - other).max() > both


def test_z_rollouts_with_forces_continue_bit_identically_and_refuse_a_floor():
    import torch
    import zroll_cases as zc
    from animsnapbases_amd import _lib
    from test_gpu_gsub import _fixture_snaps
    from test_gpu_hyper import _spec as hyper_spec
    s = zc.z_case("tris_blocks", 8, "moving")
    c = s["rf"]
    frames = np.array(s["frames"])
    N = frames.shape[1]
    snaps = _fixture_snaps(frames, 8)
    kinds, P, dt, m = [hyper_spec(c, c.ms[-1])], s["pins_dict"], s["dt"], s["masses"]
    force = fc.force_of(N)
    for mode in zc.MODES:
        kw = dict(velocity=mode, gravity=fc.G)
        ext = dict(forces=dict(force=force, start=1), pins=P)
        z, zp, F, (rec, steps) = snaps.simulate_subspace(kinds, dt, 3, 2, m, record_every=1, **ext, **kw)
        assert F == frames.shape[0] and torch.isfinite(rec).all()
        again = snaps.simulate_subspace(kinds, dt, 3, 2, m, record_every=1, **ext, **kw)
        assert torch.equal(again[0], z) and torch.equal(again[3][0], rec)
        part = snaps.simulate_subspace(kinds, dt, 3, 2, m, frame_start=3, frame_end=67, frame_jump=2, **ext, **kw)
        assert part[2] == 32 and torch.equal(part[0], z[3:67:2]) and torch.equal(part[1], zp[3:67:2])           # the rows follow the frames
        assert torch.equal(snaps.simulate_subspace(kinds, dt, 3, 2, m, chunk_frames=16, **ext, **kw)[0], z)
        for t1 in (1, 2):                                           # T1 steps continued by T2, start (and shift_start) raised by T1
            a = snaps.simulate_subspace(kinds, dt, t1, 2, m, **ext, **kw)
            assert torch.equal(a[0], rec[t1 - 1])
            b = snaps.simulate_subspace(kinds, dt, 3 - t1, 2, m, state=(a[0], a[1]), gravity=fc.G, forces=dict(force=force, start=1 + t1),
                                        pins=dict(P, shift_start=t1))
            assert torch.equal(b[0], z) and torch.equal(b[1], zp)
            stale = snaps.simulate_subspace(kinds, dt, 3 - t1, 2, m, state=(a[0], a[1]), gravity=fc.G, pins=dict(P, shift_start=t1), forces=ext["forces"])
            assert not torch.equal(stale[0], z)                     # (not raised: other rows)
        # a constant force is its row repeated; the vertices form is the same force dense; a zero table is no table
        one = snaps.simulate_subspace(kinds, dt, 3, 2, m, forces=dict(force=force[5]), **kw)[0]
        assert torch.equal(snaps.simulate_subspace(kinds, dt, 3, 2, m, forces=dict(force=np.repeat(force[5][None], 140, axis=0), start=2), **kw)[0], one)
        v = np.array([N - 1, 0, N // 2])
        dense = np.zeros_like(force)
        dense[:, v] = force[:, :3]
        assert torch.equal(snaps.simulate_subspace(kinds, dt, 3, 2, m, forces=dict(force=force[:, :3], vertices=v), **kw)[0],
                           snaps.simulate_subspace(kinds, dt, 3, 2, m, forces=dict(force=dense), **kw)[0])
        assert not torch.equal(one, snaps.simulate_subspace(kinds, dt, 3, 2, m, **kw)[0])
    # refusals: the floor at the public method, and at the C entry; a missing row before any launch; no table; a second binding
    with pytest.raises(ValueError, match="no form in the subspace coordinates"):
        snaps.simulate_subspace(kinds, dt, 3, 2, m, floor=dict(height=0.0))
    with pytest.raises(ValueError, match="row 131 of force is needed"):
        snaps.simulate_subspace(kinds, dt, 3, 2, m, forces=dict(force=force[:131]))
    eng = snaps._engine
    err = lambda: eng.lib.asb_last_error(eng.h)
    snaps.simulate_subspace(kinds, dt, 1, 1, m, forces=dict(force=force[:130]))          # a begun roll-out with its forces, rows 0 .. 129
    assert eng.lib.asb_zroll_forces(eng.h, 0) == _lib.ERR_ARG and b"already" in err()
    def state():
        bufs = [torch.empty((frames.shape[0], 8, 3), dtype=torch.float64, device="cuda:%d" % eng.device_id) for _ in range(2)]
        eng.zroll_state(bufs[0].data_ptr(), bufs[1].data_ptr())
        return bufs
    before = state()
    assert eng.lib.asb_zroll_steps(eng.h, 1, 1, 0, 0, None) == _lib.ERR_ARG and b"row 130 of the force table" in err()
    assert all(torch.equal(x, y) for x, y in zip(before, state()))          # nothing was launched
    eng.ext_set(np.zeros((7, 3 * N)), (0.0, 1))
    assert eng.lib.asb_zroll_steps(eng.h, 1, 1, 0, 0, None) == _lib.ERR_ARG and b"forces changed" in err()
    eng.ext_clear()
    assert eng.lib.asb_zroll_steps(eng.h, 1, 1, 0, 0, None) == _lib.ERR_ARG and b"forces changed" in err()
