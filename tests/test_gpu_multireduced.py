"""GPU (-m gpu): several reduced constraint kinds in one solve -- the banks of asb_rforce_bank, the per-bank slots of
asb_pdsolve_slot / asb_pdsolve_iterate, the segment table of k_hyper_apply behind asb_hyper_iterate (csrc/asb_rforce.hip,
csrc/asb_pdsolve.hip) and ``posSnapshots.set_reduced_kinds`` -- against the multi-kind host model of
tests/multireduced_cases.py (never against the device's own other path), bit for bit against themselves, and on strips against
the NumPy affine form c + sum_k G_k coef_k evaluated from the device's own previous iterate.

Shapes.  k_hyper_apply's tile is 32 vertices x 64 frames and a segment's contraction runs in steps of 4 basis vectors: fixture A
(N = 18, unions of 8 .. 18 rows) and strips of N in {3, 15, 16, 17, 31, 32, 33, 65} (unions of 3 .. 60 rows: below, at and above
the tile, ragged, N_t = N, unions larger than either kind's own set), each at F' in {1, 63, 64, 65, 130} and (m_e, m_t) in
{(1, 1), (4, 3), (1, 17), (17, 4)} where the strip allows: segments of 4 + 4, 4 + 20 and 20 + 4 contraction steps.

Bounds (tests/multireduced_cases.py, nothing fitted): one = || |A^-1| ||_inf sum_k bound_k + 64 eps kappa(A) max |q| and
B_K = 2 K max(1, amp) one, amp as stored in tests/golden/pdsolve_reduced_combined.npz.  No frame is left out.  Every measured
error is printed beside its bound.

One run on an MI355X, largest err / bound: fixture A 1.5e-5 (errors 2.2e-15 .. 1.0e-14, B_K 5.1e-10 .. 4.6e-7), the mixed solve
2.4e-5, the strips' one iteration 2.8e-3, the slab solver against the explicit inverse 4.6e-3 of 2 x 64 eps kappa(A) max |q| (a
difference of 2.2e-15) and against the host model 4.1e-8."""
import contextlib
import io

import numpy as np
import pytest

import multireduced_cases as mc
from pdsolve_cases import KS, MODES, bound_K

pytestmark = pytest.mark.gpu


def _snaps(frames, limit=2, engine=None):
    from animsnapbases_amd import posSnapshots
    kw = {} if engine is None else dict(engine=engine)
    with contextlib.redirect_stdout(io.StringIO()):
        s = posSnapshots.from_arrays(np.array(frames), None, "first", standarize=False, massWeight=False, **kw)
    if limit is not None:
        s.set_reduced_kinds(limit)
    return s


def _ops(c, ms):
    return {i: c["op"](i, m) for i, m in enumerate(ms) if m is not None}


# ------------------------------------------------------------------ 1. fixture A against the host model
@pytest.mark.parametrize("pair", mc.PAIRS_GPU)
def test_two_reduced_kinds_match_the_host_model(pair):
    a = mc.combined_case()
    z = mc.golden_combined()
    F, N = a["frames"].shape[:2]
    ops = _ops(a, pair)
    kinds = mc.reduced_specs(a, pair)
    snaps = _snaps(a["frames"])
    worst, last = 0.0, {}
    for mode in MODES:
        host = mc.model(a, range(F), mode, KS, reduced=ops)             # every frame
        for K in KS:
            amp = float(z[mc.amp_key(pair[0], pair[1], mode, K)])
            for hyper in (None, "touched", "all"):
                B = bound_K(mc.one_bound(a, ops, a["frames"], hyper is not None), K, amp)
                out, nF = snaps.solve_frames(kinds, a["dt"], K, a["masses"], velocity=mode, hyper=hyper)
                assert nF == F and tuple(out.shape) == (F, N, 3) and str(out.dtype) == "torch.float64" and out.is_cuda
                err = np.abs(out.cpu().numpy() - host[K]).max()
                print("me = %d mt = %d %s K = %d %s: max abs err %.3g, B_K %.3g, err / B_K %.3g" % (pair + (mode, K, hyper, err, B, err / B)))
                worst = max(worst, err / B)
                assert err <= B
                if K == 10 and hyper == "touched":
                    last[mode] = (out.cpu().numpy(), B)
    print("me = %d mt = %d: largest err / B_K %.3g" % (pair + (worst,)))
    assert list(snaps.assembly_ST) == ["edge_spring", "tets_strain"]
    # not vacuous: the host's solve with ONE kind reduced is further than B_K from the device's solve with both
    for mode in MODES:
        got, B = last[mode]
        for only in ({0: ops[0]}, {1: ops[1]}):
            assert np.abs(got - mc.model(a, range(F), mode, (10,), reduced=only)[10]).max() > B


def test_a_mixed_solve_matches_the_host_model():
    """Edges reduced (bank 0), tets_strain plain, tets_deformation_gradient reduced on its own basis (bank 1): the plain
    iteration with two reduced slots around a full one."""
    c = mc.mixed_case()
    z = mc.golden_combined()
    F = c["frames"].shape[0]
    ms = (mc.MIXED_MS[0], None, mc.MIXED_MS[1])
    ops = _ops(c, ms)
    snaps = _snaps(c["frames"], limit=3)
    for mode in MODES:
        host = mc.model(c, range(F), mode, KS, reduced=ops)
        for K in KS:
            B = bound_K(mc.one_bound(c, ops, c["frames"], False), K, float(z["amp_mixed_%s_%d" % (mode, K)]))
            out = snaps.solve_frames(mc.reduced_specs(c, ms), c["dt"], K, c["masses"], velocity=mode)[0]
            err = np.abs(out.cpu().numpy() - host[K]).max()
            print("mixed %s K = %d: max abs err %.3g, B_K %.3g, err / B_K %.3g" % (mode, K, err, B, err / B))
            assert err <= B
    with pytest.raises(ValueError, match="every kind reduced"):
        snaps.solve_frames(mc.reduced_specs(c, ms), c["dt"], 1, c["masses"], hyper="touched")
    plain = snaps.solve_frames(c["specs"], c["dt"], 10, c["masses"], velocity=MODES[-1])[0].cpu().numpy()
    assert np.abs(out.cpu().numpy() - plain).max() > B              # (last of the loop: MODES[-1], K = 10) the reduction is felt


# ------------------------------------------------------------------ 2. strips: one device iteration against the affine form
def _state(snaps, F, N):
    """The iterate as it lies on the device, as (F', N, 3); its padding columns are zero."""
    Q = snaps._engine.pdsolve_state(0)
    assert Q.shape[0] == 3 * N and not Q[:, F:].any()
    return np.ascontiguousarray(Q[:, :F].reshape(N, 3, F).transpose(2, 0, 1))


@pytest.mark.parametrize("n", mc.STRIPS)
def test_strips_one_iteration_is_the_affine_form(n):
    c = mc.strip_case(n)
    snaps = _snaps(c["frames"])
    worst = 0.0
    for pair in mc.strip_pairs(c, mc.STRIP_PAIRS):
        ops = _ops(c, pair)
        kinds = mc.reduced_specs(c, pair)
        nt = mc.sampled(c, ops)[0].shape[0]
        for F in mc.FRAMES:
            for hyper in ("touched", "all"):
                two = snaps.solve_frames(kinds, c["dt"], 2, c["masses"], frame_end=F, hyper=hyper)[0].cpu().numpy()
                q2 = _state(snaps, F, n)                        # the device's own iterate after two iterations
                assert np.array_equal(q2, two)
                q3 = snaps.solve_frames(kinds, c["dt"], 3, c["masses"], frame_end=F, hyper=hyper)[0].cpu().numpy()
                want = mc.affine_step(c, ops, q2, mc.affine_parts(c, ops, range(F), "difference"))
                P = {i: v[1] for i, v in mc.coefficients(c, ops, q2).items()}
                B = mc.one_bound(c, ops, q2, True, P)
                err = np.abs(q3 - want).max()
                worst = max(worst, err / B)
                assert np.isfinite(q3).all() and err <= B, (n, pair, F, hyper, err, B)
        print("strip %d, m = %s (rpp %d + %d), N_t = %d: largest err / one-iteration bound so far %.3g"
              % (n, pair, (pair[0] + 3) // 4 * 4, (pair[1] + 3) // 4 * 4, nt, worst))


# ------------------------------------------------------------------ 3. bit identity
def _identities(snaps, kinds, dt, masses, F, K=3):
    """"touched" = "all"; repeats, a sub-range, chunks of 16 frames; K iterations continued by L = K + L."""
    import torch
    kw = dict(frame_end=F)
    t = snaps.solve_frames(kinds, dt, K, masses, hyper="touched", **kw)[0]
    a = snaps.solve_frames(kinds, dt, K, masses, hyper="all", **kw)[0]
    assert torch.isfinite(t).all() and torch.equal(t, a)
    assert torch.equal(snaps.solve_frames(kinds, dt, K, masses, hyper="touched", **kw)[0], t)
    assert torch.equal(snaps.solve_frames(kinds, dt, K, masses, hyper="touched", chunk_frames=16, **kw)[0], t)
    assert torch.equal(snaps.solve_frames(kinds, dt, K, masses, hyper="all", chunk_frames=16, **kw)[0], t)
    plain = snaps.solve_frames(kinds, dt, K, masses, **kw)[0]
    assert torch.equal(snaps.solve_frames(kinds, dt, K, masses, chunk_frames=16, **kw)[0], plain)
    if F > 3:
        part, nF = snaps.solve_frames(kinds, dt, K, masses, hyper="touched", frame_start=1, frame_end=F, frame_jump=2)
        assert nF == len(range(1, F, 2)) and torch.equal(part, t[1:F:2])
        assert torch.equal(snaps.solve_frames(kinds, dt, K, masses, frame_start=1, frame_end=F, frame_jump=2)[0], plain[1:F:2])
    for k, l in ((1, 2), (2, 1)):
        first = snaps.solve_frames(kinds, dt, k, masses, hyper="touched", **kw)[0]
        keep = first.clone()
        assert torch.equal(snaps.solve_frames(kinds, dt, l, masses, start=first, hyper="all", **kw)[0], t)
        assert torch.equal(snaps.solve_frames(kinds, dt, l, masses, start=first, hyper="touched", **kw)[0], t)
        assert torch.equal(first, keep)
    return t


def test_bit_identity_on_fixture_a():
    import torch
    a = mc.combined_case()
    snaps = _snaps(a["frames"])
    F = a["frames"].shape[0]
    outs = [_identities(snaps, mc.reduced_specs(a, pair), a["dt"], a["masses"], F) for pair in ((1, 17), (17, 1))]
    assert not torch.equal(outs[0], outs[1])
    assert not torch.equal(snaps.solve_frames(mc.reduced_specs(a, (17, 1)), a["dt"], 1, a["masses"], hyper="touched")[0], outs[1])


@pytest.mark.parametrize("n", [17, 33, 65])
def test_bit_identity_on_strips(n):
    c = mc.strip_case(n)
    snaps = _snaps(c["frames"])
    for pair in mc.strip_pairs(c, [(4, 3), (17, 4)]):
        for F in (1, 65, 130):
            _identities(snaps, mc.reduced_specs(c, pair), c["dt"], c["masses"], F)


def test_rollouts_continue_bit_for_bit():
    """T1 steps then T2 through state= equal T1 + T2, with and without hyper; step 1 is solve_frames; records as ever."""
    import torch
    c = mc.strip_case(33)
    kinds = mc.reduced_specs(c, (4, 3))
    snaps = _snaps(c["frames"])
    kw = dict(num_iterations=3, masses=c["masses"], frame_start=2, frame_end=100, frame_jump=3)
    for hyper in (None, "touched", "all"):
        q, qp, nF, (rec, steps) = snaps.simulate_frames(kinds, c["dt"], 5, record_every=2, hyper=hyper, **kw)
        assert steps == [2, 4] and torch.isfinite(q).all()
        q2, qp2, _ = snaps.simulate_frames(kinds, c["dt"], 2, hyper=hyper, **kw)
        assert torch.equal(q2, rec[0])
        q5, qp5, _ = snaps.simulate_frames(kinds, c["dt"], 3, state=(q2, qp2), hyper=hyper, chunk_frames=16, **kw)
        assert torch.equal(q5, q) and torch.equal(qp5, qp) and torch.equal(qp5, snaps.simulate_frames(kinds, c["dt"], 4, hyper=hyper, **kw)[0])
        q1 = snaps.simulate_frames(kinds, c["dt"], 1, hyper=hyper, **kw)[0]
        sel = {k: v for k, v in kw.items() if k.startswith("frame")}
        assert torch.equal(q1, snaps.solve_frames(kinds, c["dt"], 3, c["masses"], hyper=hyper, **sel)[0])
    t = snaps.simulate_frames(kinds, c["dt"], 4, hyper="touched", **kw)[0]
    assert torch.equal(t, snaps.simulate_frames(kinds, c["dt"], 4, hyper="all", **kw)[0])


def test_a_solve_after_one_of_another_shape_equals_a_fresh_context():
    import torch
    small, big = mc.strip_case(33), mc.strip_case(65)
    ks, kb = mc.reduced_specs(small, (4, 3)), mc.reduced_specs(big, (17, 4))
    fresh = _snaps(small["frames"][:70]).solve_frames(ks, small["dt"], 3, small["masses"], hyper="touched")[0]
    first = _snaps(big["frames"][:5])
    first.solve_frames(kb, big["dt"], 2, big["masses"], hyper="touched")
    again = _snaps(small["frames"][:70], engine=first._engine)
    assert again._engine is first._engine
    assert torch.equal(again.solve_frames(ks, small["dt"], 3, small["masses"], hyper="touched")[0], fresh)
    # on one tensor: the kinds in the other order (the banks change hands), a one-kind solve and the plain path in between
    snaps = _snaps(big["frames"])
    want = _snaps(big["frames"]).solve_frames(mc.reduced_specs(big, (3, 4)), big["dt"], 2, big["masses"], frame_end=7, hyper="touched")[0]
    snaps.solve_frames(kb[::-1], big["dt"], 2, big["masses"], hyper="all")
    snaps.solve_frames(kb[1:], big["dt"], 2, big["masses"], hyper="touched")
    snaps.solve_frames(kb, big["dt"], 1, big["masses"])
    assert torch.equal(snaps.solve_frames(mc.reduced_specs(big, (3, 4)), big["dt"], 2, big["masses"], frame_end=7, hyper="touched")[0], want)


def test_one_reduced_kind_under_a_raised_limit_keeps_its_bits():
    import torch
    from hyper_cases import chain_case
    c = chain_case(33)
    spec = dict(c["spec"], basis=c["basis"], num_components=4)
    for hyper in ("touched", "all", None):
        want = _snaps(c["frames"], limit=None).solve_frames([spec], c["dt"], 3, c["masses"], hyper=hyper)[0]
        snaps = _snaps(c["frames"], limit=8)
        assert torch.equal(snaps.solve_frames([spec], c["dt"], 3, c["masses"], hyper=hyper)[0], want)
    # ... also after a two-kind solve on the same object has used bank 1
    s = mc.strip_case(33)
    snaps = _snaps(s["frames"], limit=8)
    one = mc.reduced_specs(s, (4, None))
    want = _snaps(s["frames"], limit=None).solve_frames(one, s["dt"], 3, s["masses"])[0]
    snaps.solve_frames(mc.reduced_specs(s, (17, 4)), s["dt"], 2, s["masses"], hyper="touched")
    assert torch.equal(snaps.solve_frames(one, s["dt"], 3, s["masses"])[0], want)


# ------------------------------------------------------------------ 4. the C layer
def test_refusals_at_the_c_layer():
    import torch
    from animsnapbases_amd import projections as proj
    a = mc.combined_case()
    pair = (4, 17)
    ops = _ops(a, pair)
    kinds = mc.reduced_specs(a, pair)
    N = a["frames"].shape[1]
    dt, m = a["dt"], a["masses"]
    snaps = _snaps(a["frames"])
    eng = snaps._engine
    for bad in (8, -1, 1 << 20):
        with pytest.raises(RuntimeError, match="bank"):
            eng.rforce_bank(bad)
    with pytest.raises(ValueError, match="set_reduced_kinds"):
        snaps.set_reduced_kinds(9)
    good = snaps.solve_frames(kinds, dt, 2, m, frame_end=4, hyper="touched")[0]
    # the solve above left the inverse, and per bank S^T V, the solver and G, on the device; bank 0 is current
    union, compact, _ = mc.sampled(a, ops)

    def slot(i, bank):
        eng.rforce_bank(bank)
        eng.cproj_setup(compact[i])
        eng.rforce_solver(ops[i].H, ops[i].local_rows)
        eng.pdsolve_slot(a["kinds"][i][2], a["kinds"][i][3], None)

    def begin(banks=(0, 1)):
        eng.pdsolve_begin(0, 0, 4, 1, None, False, 1.0, m / dt ** 2, 1, np.zeros(3), 0)
        for i, b in enumerate(banks):
            slot(i, b)
        eng.rforce_bank(0)
    out = torch.empty_like(good)
    begin()
    eng.hyper_iterate(2, union, 0, out.data_ptr())
    assert torch.equal(out, good)
    # a reduced slot on a bank this solve has bound already
    eng.pdsolve_begin(0, 0, 4, 1, None, False, 1.0, m / dt ** 2, 1, np.zeros(3), 0)
    slot(0, 0)
    eng.cproj_setup(compact[1])
    with pytest.raises(RuntimeError, match="second reduced kind"):
        eng.pdsolve_slot(1.0, 1.0, None)
    eng.rforce_bank(1)
    eng.cproj_setup(compact[1])
    eng.pdsolve_slot(a["kinds"][1][2], a["kinds"][1][3], None)             # ... and on its own bank it is taken
    eng.rforce_bank(0)
    eng.hyper_iterate(2, union, 0, out.data_ptr())
    assert torch.equal(out, good)
    # a slot whose tables name a vertex past the union's length; a list that is not ascending
    begin()
    with pytest.raises(RuntimeError, match="names vertex"):
        eng.hyper_iterate(1, union[:-1])
    with pytest.raises(RuntimeError, match="ascending"):
        eng.hyper_iterate(1, union[::-1])
    # a slot that is not reduced beside a reduced one
    eng.pdsolve_begin(0, 0, 4, 1, None, False, 1.0, m / dt ** 2, 1, np.zeros(3), 0)
    slot(0, 0)
    eng.cproj_setup(a["kinds"][1][0])
    eng.pdsolve_slot(a["kinds"][1][2], a["kinds"][1][3], a["kinds"][1][1])
    with pytest.raises(RuntimeError, match="every kind must be reduced"):
        eng.hyper_iterate(1, None)
    # a stale G on bank 1: after another matrix (every bank's mark is cleared) ...
    eng.gstep_setup(proj.global_matrix([(k[0], 0.7) for k in a["kinds"]], N, m, 2 * dt))
    begin()
    with pytest.raises(RuntimeError, match="stale"):
        eng.hyper_iterate(1, union)
    eng.gstep_setup(a["A"])
    eng.hyper_operator()                                                    # bank 0 alone is formed again: bank 1 stays stale
    begin()
    with pytest.raises(RuntimeError, match="stale"):
        eng.hyper_iterate(1, union)
    eng.rforce_bank(1)
    eng.hyper_operator()
    eng.rforce_bank(0)
    begin()
    eng.hyper_iterate(2, union, 0, out.data_ptr())
    assert torch.equal(out, good)
    # ... and after rforce_operator on bank 1 alone: bank 0's G survives, bank 1's does not
    eng.rforce_bank(1)
    eng.rforce_operator(a["kinds"][1][1], ops[1].V)
    eng.rforce_bank(0)
    begin()
    with pytest.raises(RuntimeError, match="stale"):
        eng.hyper_iterate(1, union)
    eng.rforce_bank(1)
    eng.hyper_operator()                                                    # bank 1 alone: bank 0's G was never touched
    eng.rforce_bank(0)
    begin()
    eng.hyper_iterate(2, union, 0, out.data_ptr())
    assert torch.equal(out, good)
    # the plain iteration notices a bank whose operator went: "changed since asb_pdsolve_slot"
    begin()
    eng.rforce_bank(1)
    eng.rforce_operator(a["kinds"][1][1], ops[1].V)                         # (drops the solver of bank 1)
    eng.rforce_bank(0)
    with pytest.raises(RuntimeError, match="changed since asb_pdsolve_slot"):
        eng.pdsolve_iterate(1)
    assert torch.equal(snaps.solve_frames(kinds, dt, 2, m, frame_end=4, hyper="all")[0], good)


# ------------------------------------------------------------------ 5. the slab solver
def test_two_reduced_kinds_under_the_slab_solver():
    """One solve of fixture A under the block-tridiagonal factor, held to the agreement ``set_global_solver`` documents: each
    solver within 64 eps kappa(A) max |q| of the exact solve.  At K = 1 both solvers start from the same iterate, so the
    projections and coefficients they see are the same bits and only the application of A^-1 differs: the two results lie within
    2 x 64 eps kappa(A) max |q| of each other, with and without ``hyper`` (there A^-1 enters through c and G; max |q| of the
    result is kept as the scale, the issue's bound, not the larger max |c| + sum |G| |coef|).  In addition every solve is
    within B_K of the host model."""
    a = mc.combined_case()
    z = mc.golden_combined()
    F = a["frames"].shape[0]
    pair = (4, 17)
    ops = _ops(a, pair)
    kinds = mc.reduced_specs(a, pair)
    inverse = _snaps(a["frames"])
    slab = _snaps(a["frames"])
    slab.set_global_solver("slab", slab_target=8)
    host = mc.model(a, range(F), "difference", KS, reduced=ops)
    for K in (1, 3):
        for hyper in (None, "touched", "all"):
            got = slab.solve_frames(kinds, a["dt"], K, a["masses"], hyper=hyper)[0].cpu().numpy()
            if K == 1:
                other = inverse.solve_frames(kinds, a["dt"], K, a["masses"], hyper=hyper)[0].cpu().numpy()
                agree = 2 * 64 * mc.EPS * a["kappa"] * np.abs(host[K]).max()
                diff = np.abs(got - other).max()
                print("slab against inverse, K = 1 %s: max abs difference %.3g, 2 x 64 eps kappa max|q| = %.3g, ratio %.3g"
                      % (hyper, diff, agree, diff / agree))
                assert diff <= agree
            B = bound_K(mc.one_bound(a, ops, a["frames"], hyper is not None), K, float(z[mc.amp_key(pair[0], pair[1], "difference", K)]))
            err = np.abs(got - host[K]).max()
            print("slab K = %d %s: max abs err %.3g, B_K %.3g, err / B_K %.3g" % (K, hyper, err, B, err / B))
            assert err <= B
    assert slab.global_solve_slabs[0] >= 2
