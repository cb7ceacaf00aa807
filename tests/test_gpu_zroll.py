"""GPU (-m gpu): roll-outs whose state lives in the coordinates z of a position subspace (csrc/asb_zroll.hip) --
the affine product kernel alone, ``subspace_coordinates`` / ``subspace_expand``, ``simulate_subspace`` against the longdouble model
of tests/zroll_model.py, cross-checks against ``simulate_frames(hyper="touched")``, two reduced kinds, the bit identities, the
refusals.  Bounds: tests/zroll_cases.py derives them; every measured err / bound is printed; no frame, record or case is left out.

1. ``asb_test_zroll_affine``: r in {1, 3, 4, 17, 33} rows (rq 16, 32, 48), contraction lengths {1, 3, 4, 5, 17}, one segment and two of
   unequal length, widths {1, 63, 64, 65, 130}, base per entry and broadcast.  Bound (len + 16) eps (|base| + sum |M| |X|): the
   base is one more term of the sum (fl(base + acc) rounds relative to it).
2. Coordinates and expansion on chains N in {2, 15, 16, 17, 31, 32, 33, 65} and on a fixture through the public methods.
3. Roll-outs against the model, every record, in z and expanded.  4. Against the parent's paths.  5. Two reduced kinds.
6. Bit identities.  7. Refusals.  Every test fails on the parent commit, where the methods and symbols do not exist.

Largest err / bound measured on an MI355X: 1. 0.117; 2. chains 0.273, public 0.080, expand(coordinates(x)) 0.031; 3. tris_blocks 2.9e-4,
tets_deim 3.1e-6, pinned 1.1e-4; 4. projected frames 1.2e-5, r = N under "inverse" 9.1e-6; 5. 1.0e-6 (also in DESIGN.md 3.21)."""
import numpy as np
import pytest

import gsub_cases as gc
import hyper_cases as hc
import pdsolve_cases as pc
import pins_cases as pins
import rollout_cases as rc
import zroll_cases as zc
from gslab_model import chain_matrix
from gsub_model import EPS, LD, svd_basis
from test_gpu_gsub import CHAINS, RS, WIDTHS, _fb, _fixture_snaps, _hyper_parts, _snaps
from test_gpu_hyper import _spec as hyper_spec
from zroll_model import ZModel

pytestmark = pytest.mark.gpu

LENS = [1, 3, 4, 5, 17]
SELKW = dict(frame_jump=3)                              # range(0, 130, 3): rollout_cases.START_FRAMES


def _plain(spec):
    return {k: v for k, v in spec.items() if k not in ("basis", "num_components", "reduction")}


def _dev(eng, a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:%d" % eng.device_id)


# ------------------------------------------------------------------ 1. the product kernel alone
@pytest.mark.parametrize("r", [1, 3, 4, 17, 33])
def test_affine_product_kernel(r):
    rng = np.random.default_rng(700 + r)
    eng = _snaps(rng.standard_normal((2, 5, 3)))._engine
    rq = (r + 15) // 16 * 16
    worst = 0.0
    for li, L in enumerate(LENS):
        for lens in ((L,), (L, LENS[(li + 2) % len(LENS)])):
            W = max(WIDTHS)
            Ms = [rng.standard_normal((3, r, k)) * 10.0 ** rng.integers(-2, 3, size=(3, r, 1)) for k in lens]
            Xs = [rng.standard_normal((3, k, W)) * 10.0 ** rng.integers(-2, 3, size=(3, k, 1)) for k in lens]
            for bcast in (False, True):
                base = rng.standard_normal((3, r) if bcast else (3, r, W))
                wide = None
                for w in sorted(WIDTHS, reverse=True):
                    b = base if bcast else base[:, :, :w]
                    got = eng.zroll_affine(Ms, [X[:, :, :w] for X in Xs], b)
                    assert got.shape == (3, rq, (w + 63) // 64 * 64)
                    bb = (b[:, :, None] if bcast else b).astype(LD)
                    ref = bb + sum(np.einsum("djk,dkf->djf", M.astype(LD), X[:, :, :w].astype(LD)) for M, X in zip(Ms, Xs))
                    mag = np.abs(bb).astype(np.float64) + sum(np.einsum("djk,dkf->djf", np.abs(M), np.abs(X[:, :, :w])) for M, X in zip(Ms, Xs))
                    err = np.abs(got[:, :r, :w] - ref).astype(np.float64)
                    bnd = (sum(lens) + 16) * EPS * mag
                    worst = max(worst, float((err / bnd).max()))
                    assert (err <= bnd).all(), (r, lens, w, bcast, float((err / bnd).max()))
                    assert not got[:, r:, :].any()                                          # the padding rows: zero operands
                    if not bcast:
                        assert not got[:, :, w:].any()                                      # and columns
                    if wide is None:
                        wide = got
                    assert np.array_equal(got[:, :r, :w], wide[:, :r, :w])                  # a column does not depend on its neighbours
    print("affine product r = %d: largest err / bound %.3g" % (r, worst))
    assert worst < 1.0


# ------------------------------------------------------------------ 2. coordinates and expansion
def _coord_bound(zm, x):
    """(F, r, 3): (N + 2) eps |U^T| |x - o|, the chain over N and the subtraction."""
    g = zm.g
    return np.stack([(g.N + 2) * EPS * (np.abs(x[:, :, d] - g.o[None, :, d].astype(np.float64)) @ np.abs(g.U[d]).astype(np.float64))
                     for d in range(3)], axis=2)


def _expand_bound(zm, z):
    """(F, N, 3): (r + 2) eps (|o| + |U| |z|)."""
    g = zm.g
    return np.stack([(g.r + 2) * EPS * (np.abs(g.o[None, :, d]).astype(np.float64) + np.abs(z[:, :, d]) @ np.abs(g.U[d]).astype(np.float64).T)
                     for d in range(3)], axis=2)


class _Lin(object):
    """What ``ZModel.coordinates`` / ``expand`` read of a model, for a bare basis."""
    def __init__(self, g):
        self.g = g
    coordinates, expand = ZModel.coordinates, ZModel.expand


@pytest.mark.parametrize("n", CHAINS)
def test_coordinates_and_expansion_on_chains(n):
    from animsnapbases_amd import projections as proj
    from gsub_model import Galerkin
    import torch
    rng = np.random.default_rng(800 + n)
    A = chain_matrix(n)
    eng = _snaps(rng.standard_normal((2, n, 3)))._engine
    comps, origin = rng.standard_normal((n, n, 3)), rng.standard_normal((n, 3))
    W = max(WIDTHS)
    x = rng.standard_normal((W, n, 3)) * 10.0 ** rng.integers(-2, 3, size=(1, n, 1))
    worst = 0.0
    for r in sorted(set(k for k in RS + [n] if k <= n)):
        Qt = proj.subspace_basis(comps, r)
        eng.gsub_setup(A, Qt, origin)
        lin = _Lin(Galerkin(A, Qt, origin))
        zin = rng.standard_normal((W, r, 3))
        wide = None
        for w in sorted(WIDTHS, reverse=True):
            xd, zd = _dev(eng, x[:w]), _dev(eng, zin[:w])
            z = torch.full((w, r, 3), float("nan"), dtype=torch.float64, device=xd.device)
            q = torch.full((w, n, 3), float("nan"), dtype=torch.float64, device=xd.device)
            eng.gsub_coordinates(0, 0, 1, 1, None, False, 1.0, z.data_ptr(), xd.data_ptr(), w)
            eng.gsub_expand(zd.data_ptr(), w, q.data_ptr())
            z, q = z.cpu().numpy(), q.cpu().numpy()
            assert np.isfinite(z).all() and np.isfinite(q).all()
            ez, bz = np.abs(z - lin.coordinates(x[:w])).astype(np.float64), _coord_bound(lin, x[:w])
            eq, bq = np.abs(q - lin.expand(zin[:w].astype(LD))).astype(np.float64), _expand_bound(lin, zin[:w])
            worst = max(worst, float((ez / bz).max()), float((eq / bq).max()))
            assert (ez <= bz).all() and (eq <= bq).all(), (n, r, w, float((ez / bz).max()), float((eq / bq).max()))
            if wide is None:
                wide = (z, q)
            assert np.array_equal(z, wide[0][:w]) and np.array_equal(q, wide[1][:w])       # a frame does not depend on its neighbours
    print("chain %d coordinates / expansion: largest err / bound %.3g" % (n, worst))
    assert worst < 1.0


def test_coordinates_and_expansion_through_the_public_methods():
    import torch
    s = zc.z_case("tris_blocks", 8)
    zm = ZModel(s, {0: zc.operator(s, 3)})
    frames = np.array(s["frames"])
    snaps = _fixture_snaps(frames, 8)
    with pytest.raises(ValueError, match="no position subspace on the device"):
        snaps.subspace_coordinates("train")
    snaps.global_solve_setup([_plain(hyper_spec(s["rf"], 3))], s["dt"], s["masses"])
    z = snaps.subspace_coordinates("train")
    F = frames.shape[0]
    assert tuple(z.shape) == (F, 8, 3) and z.is_cuda and z.dtype == torch.float64
    ref = zm.coordinates(frames)
    # (the resident tensor is scaled: x comes back as fl(T / psf), one more eps |x| through |U^T|)
    bz = _coord_bound(zm, frames) + EPS * np.stack([np.abs(frames[:, :, d]) @ np.abs(zm.g.U[d]).astype(np.float64) for d in range(3)], axis=2)
    ez = np.abs(z.cpu().numpy() - ref).astype(np.float64)
    print("public coordinates: largest err / bound %.3g" % float((ez / bz).max()))
    assert (ez <= bz).all()
    assert torch.equal(snaps.subspace_coordinates("train", 3, 67, 2), z[3:67:2])
    given = snaps.subspace_coordinates(_dev(snaps._engine, frames))
    assert (np.abs(given.cpu().numpy() - ref).astype(np.float64) <= _coord_bound(zm, frames)).all()
    snaps.test_verts = frames[5:40]
    assert torch.equal(snaps.subspace_coordinates("test"), snaps.subspace_coordinates(_dev(snaps._engine, frames[5:40])))
    # an x built in the span comes back: coordinates' bound through |U|, the expansion's, and x's own rounding (eps / 2 |x|)
    zs = np.random.default_rng(3).standard_normal((70, 8, 3))
    x = zm.expand(zs.astype(LD)).astype(np.float64)
    back = snaps.subspace_expand(snaps.subspace_coordinates(_dev(snaps._engine, x))).cpu().numpy()
    zb = _coord_bound(zm, x) + 0.5 * EPS * np.stack([np.abs(x[:, :, d]) @ np.abs(zm.g.U[d]).astype(np.float64) for d in range(3)], axis=2)
    bnd = _expand_bound(zm, zs) + np.stack([zb[:, :, d] @ np.abs(zm.g.U[d]).astype(np.float64).T for d in range(3)], axis=2)
    err = np.abs(back - x)
    print("expand(coordinates(x)): largest err / bound %.3g" % float((err / bnd).max()))
    assert (err <= bnd).all()
    for bad in (z.cpu(), z.float(), z[:, :4], z.transpose(0, 1)):
        with pytest.raises(ValueError, match="subspace_expand"):
            snaps.subspace_expand(bad)
    with pytest.raises(ValueError, match="subspace_coordinates"):
        snaps.subspace_coordinates(_dev(snaps._engine, frames[:, :5]))


# ------------------------------------------------------------------ 3. roll-outs against the host model
def _unorm(zm):
    """max_d || |U_d^T| ||_inf: |e_z| = |U^T (U e_z)| <= this times max |U e_z| (U^T U = I to 16 eps)."""
    return max(float(np.abs(zm.g.U[d]).astype(np.float64).sum(axis=0).max()) for d in range(3)) * (1.0 + 64 * EPS * zm.g.r)


def _check_rollout(tag, snaps, zm, s, kinds, ops, K, T, mode, amp, P=None, gravity=None):
    """One ``simulate_subspace`` with every record against the model: z directly and expanded.  Returns (worst ratio, B_T, q_T)."""
    kw = dict(SELKW)
    if gravity is not None:
        kw["gravity"] = gravity
    z, zp, nF, (rec, steps) = snaps.simulate_subspace(kinds, s["dt"], T, K, s["masses"], velocity=mode, pins=P, record_every=1, **kw)
    assert nF == len(zc.SEL) and steps == list(range(1, T + 1)) and tuple(rec.shape) == (T, nF, zm.g.r, 3)
    x = s["frames"][zc.SEL]
    zs, recs = zm.rollout(*zm.start(s["frames"], zc.SEL, mode), K, T, None if P is None else np.array(zc.SEL))
    B = zc.bounds(zm, recs, K, amp, zc.conds_of(ops), 3 * zc.start_bound(zm, x))
    got = rec.cpu().numpy()
    assert np.array_equal(got[-1], z.cpu().numpy())
    if T > 1:
        assert np.array_equal(got[-2], zp.cpu().numpy())
    worst, un = 0.0, _unorm(zm)
    for t in range(T):
        ez = float(np.abs(got[t] - zs[t]).max())
        q = snaps.subspace_expand(rec[t]).cpu().numpy()
        qm = zm.expand(zs[t])
        eq = float(np.abs(q - qm).max())
        Bq = B[t] + float(_expand_bound(zm, got[t]).max())
        print("%s step %d: |dz| %.3g (bound %.3g), |dq| %.3g (bound %.3g), err / bound %.3g" % (tag, t + 1, ez, un * B[t], eq, Bq, max(ez / (un * B[t]), eq / Bq)))
        assert ez <= un * B[t] and eq <= Bq
        worst = max(worst, ez / (un * B[t]), eq / Bq)
    move = float(np.abs(q - x).max())
    assert move > 1e6 * B[-1], (tag, move, B[-1])                                           # not vacuous: the roll-out went somewhere
    return worst, B[-1], q


@pytest.mark.parametrize("fixture,r,m,K,T", zc.FREE)
def test_rollouts_match_the_host_model(fixture, r, m, K, T):
    s = zc.z_case(fixture, r)
    op = zc.operator(s, m)
    zm = ZModel(s, {0: op})
    snaps = _fixture_snaps(np.array(s["frames"]), r)
    worst = 0.0
    for mode in zc.MODES:
        amp = zc.amp_of(s, m, mode, K, T)
        tag = "%s r = %d m = %d K = %d %s" % (fixture, r, m, K, mode)
        worst = max(worst, _check_rollout(tag, snaps, zm, s, [hyper_spec(s["rf"], m)], {0: op}, K, T, mode, amp)[0])
    print("roll-outs %s r = %d m = %d K = %d T = %d: largest err / bound %.3g" % (fixture, r, m, K, T, worst))


@pytest.mark.parametrize("fixture,pn,r,m,K,T", zc.PINNED)
def test_pinned_rollouts_match_the_host_model(fixture, pn, r, m, K, T):
    s = zc.z_case(fixture, r, pn)
    op = zc.operator(s, m)
    acc = s["dt"] ** 2 * np.array(pins.G)
    zm = ZModel(s, {0: op}, acc)
    snaps = _fixture_snaps(np.array(s["frames"]), r)
    kinds, P = [hyper_spec(s["rf"], m)], s["pins_dict"]
    worst = 0.0
    for mode in zc.MODES:
        amp = zc.amp_of(s, m, mode, K, T, acc)
        tag = "%s %s pins r = %d m = %d K = %d %s" % (fixture, pn, r, m, K, mode)
        w, B, q = _check_rollout(tag, snaps, zm, s, kinds, {0: op}, K, T, mode, amp, P, pins.G)
        worst = max(worst, w)
        # without the pins, and without gravity, the roll-out is somewhere else by more than the bound
        kw = dict(velocity=mode, **SELKW)
        loose = snaps.subspace_expand(snaps.simulate_subspace(kinds, s["dt"], T, K, s["masses"], gravity=pins.G, **kw)[0]).cpu().numpy()
        still = snaps.subspace_expand(snaps.simulate_subspace(kinds, s["dt"], T, K, s["masses"], pins=P, **kw)[0]).cpu().numpy()
        assert np.abs(loose - q).max() > B and np.abs(still - q).max() > B
    print("pinned roll-outs %s %s: largest err / bound %.3g" % (fixture, pn, worst))


# ------------------------------------------------------------------ 4. against the parent's paths
@pytest.mark.parametrize("fixture", ["tets_deim", "tris_blocks"])
def test_on_projected_frames_it_is_the_hyper_rollout_under_the_subspace(fixture):
    """The animation projected into o + span(U) on the host: ``subspace_expand(z_T)`` and ``simulate_frames(hyper="touched")``
    under "subspace" compute the same roll-out; each lies within its own bound of the exact one.  The parent's bound is the one
    of tests/test_gpu_gsub.py (``hyper_bound`` and the reduced-force bound with N more terms) with kappa_d = 0 in the latter, as
    ``zroll_cases.conds_of`` argues: both device paths and the exact recurrence multiply by the same explicit H_d."""
    from hyper_cases import reduced_force_bound
    r, K, T = 8, 3, 2
    s0 = zc.z_case(fixture, r)
    c = s0["rf"]
    m = c.ms[-1]
    op = zc.operator(s0, m)
    s = dict(s0, frames=s0["proj_frames"])
    g = s["galerkin"]
    zm = ZModel(s, {0: op})
    snaps = _snaps(s["frames"], svd_basis(s0["frames"]), r, np.array(s0["frames"][0]))
    spec = [hyper_spec(c, m)]
    pinf, fb = gc.p_abs_inf(g), _fb(c.kind)
    redb = float(reduced_force_bound(c.St, op, c.p_pt(m), np.zeros(3), zc.RAW_TOL, c.St.shape[0]).max())
    for mode in zc.MODES:
        amp = zc.amp_of(s0, m, mode, K, T)
        zs, recs = zm.rollout(*zm.start(s["frames"], zc.SEL, mode), K, T)
        mine = zc.bounds(zm, recs, K, amp, zc.conds_of({0: op}), 3 * zc.start_bound(zm, s["frames"][zc.SEL]))[-1]
        sq, sp = rc.start_state(s["frames"], zc.SEL, mode)
        host = rc.rollout(s, K, T, sq, sp, reduced=(0, op))
        ms, M, coef = _hyper_parts(s, c, op, host[0], rc.carry(host[0], sp)[0])
        one = pinf * max(fb, redb) + gc.hyper_bound(g, ms, M, coef, np.abs(host[1]).max())
        theirs = rc.bound_T(one, K, T, float(amp[-1]), rc.adv_bound(host[1], host[1]))
        z = snaps.simulate_subspace(spec, s["dt"], T, K, s["masses"], velocity=mode, **SELKW)[0]
        q = snaps.subspace_expand(z).cpu().numpy()
        parent = snaps.simulate_frames(spec, s["dt"], T, K, s["masses"], velocity=mode, hyper="touched", **SELKW)[0].cpu().numpy()
        both = mine + float(_expand_bound(zm, z.cpu().numpy()).max()) + theirs
        err = float(np.abs(q - parent).max())
        print("%s %s projected frames: |z roll-out - hyper roll-out| %.3g, bound %.3g + %.3g, err / bound %.3g" % (fixture, mode, err, mine, theirs, err / both))
        assert err <= both
        assert np.abs(q - s["frames"][zc.SEL]).max() > 1e6 * both


@pytest.mark.parametrize("fixture", ["tets_deim", "tris_blocks"])
def test_with_the_full_basis_it_is_the_hyper_rollout_under_the_inverse(fixture):
    """r = N and the frames as they are: the Galerkin step is A^-1, so the roll-out in z is the hyper-reduced roll-out under
    "inverse", T = 2.  The parent's bound: ``hyper_cases.one_bound`` as tests/test_gpu_hyper.py takes it, with kappa_d = 0
    (``zroll_cases.conds_of``)."""
    K, T = 3, 2
    s = zc.z_case(fixture, None)
    c = s["rf"]
    m = c.ms[-1]
    op = zc.operator(s, m)
    zm = ZModel(s, {0: op})
    full = pc.host_case(c.kind)
    dc = hc.of_host_case(full)
    frames = np.array(s["frames"])
    snaps, inv = _fixture_snaps(frames, None), _snaps(frames)
    spec = [hyper_spec(c, m)]
    for mode in zc.MODES:
        amp = rc.measure_amp(full, mode, K, T, zc.SEL, reduced=(0, op))
        zs, recs = zm.rollout(*zm.start(frames, zc.SEL, mode), K, T)
        mine = zc.bounds(zm, recs, K, amp, zc.conds_of({0: op}), 3 * zc.start_bound(zm, frames[zc.SEL]))[-1]
        sq, sp = rc.start_state(full["frames"], zc.SEL, mode)
        host = rc.rollout(full, K, T, sq, sp, reduced=(0, op))
        one = hc.one_bound(dc["Ainv_abs_inf"], dc["kappa"], c.St, op, c.p_pt(m), np.zeros(3), _fb(c.kind), zc.RAW_TOL, np.abs(host[1]).max())
        theirs = rc.bound_T(one, K, T, float(amp[-1]), rc.adv_bound(host[1], host[1]))
        z = snaps.simulate_subspace(spec, s["dt"], T, K, s["masses"], velocity=mode, **SELKW)[0]
        q = snaps.subspace_expand(z).cpu().numpy()
        other = inv.simulate_frames(spec, s["dt"], T, K, s["masses"], velocity=mode, hyper="touched", **SELKW)[0].cpu().numpy()
        both = mine + float(_expand_bound(zm, z.cpu().numpy()).max()) + theirs
        err = float(np.abs(q - other).max())
        print("%s %s r = N: |z roll-out - hyper roll-out under inverse| %.3g, bound %.3g + %.3g, err / bound %.3g" % (fixture, mode, err, mine, theirs, err / both))
        assert err <= both
        assert np.abs(q - frames[zc.SEL]).max() > 1e6 * both


# ------------------------------------------------------------------ 5. two reduced kinds
def test_two_reduced_kinds():
    import multireduced_cases as mc
    a = mc.combined_case()
    pair, r, K, T = (4, 17), 8, 3, 2
    s = gc.sub_case("combined", r)
    ops = {i: a["op"](i, mi) for i, mi in enumerate(pair)}
    zm = ZModel(s, ops)
    frames = np.array(s["frames"])
    snaps = _fixture_snaps(frames, r)
    snaps.set_reduced_kinds(2)
    kinds = mc.reduced_specs(a, pair)
    proj = dict(s, frames=zm.project(frames))
    worst = 0.0
    for mode in zc.MODES:
        amp = zc.measure_amp_multi(proj, mode, K, T, ops)
        worst = max(worst, _check_rollout("two kinds %s" % mode, snaps, zm, s, kinds, ops, K, T, mode, amp)[0])
    # not vacuous: one kind alone is another roll-out
    both = snaps.simulate_subspace(kinds, s["dt"], T, K, s["masses"], **SELKW)[0]
    print("two reduced kinds: largest err / bound %.3g" % worst)
    assert list(snaps.assembly_ST) == ["edge_spring", "tets_strain"]
    assert float((snaps.simulate_subspace(kinds[1:], s["dt"], T, K, s["masses"], **SELKW)[0] - both).abs().max()) > 1e-3


# ------------------------------------------------------------------ 6. bit identities
@pytest.mark.parametrize("fixture,pn", [("tris_blocks", None), ("tets_deim", "moving")])
def test_bit_identities(fixture, pn):
    import torch
    s = zc.z_case(fixture, 8, pn)
    c = s["rf"]
    frames = np.array(s["frames"])
    snaps = _fixture_snaps(frames, 8)
    kinds, P, dt, m = [hyper_spec(c, c.ms[-1])], s["pins_dict"], s["dt"], s["masses"]
    g = (0.0, 0.0, 0.0) if pn is None else pins.G
    for mode in zc.MODES:
        kw = dict(velocity=mode, gravity=g, pins=P)
        z, zp, F, (rec, steps) = snaps.simulate_subspace(kinds, dt, 3, 2, m, record_every=1, **kw)
        assert F == frames.shape[0] and torch.isfinite(rec).all()
        again = snaps.simulate_subspace(kinds, dt, 3, 2, m, record_every=1, **kw)
        assert torch.equal(again[0], z) and torch.equal(again[1], zp) and torch.equal(again[3][0], rec)         # repeats
        assert torch.equal(rec[-1], z) and torch.equal(rec[-2], zp)
        part = snaps.simulate_subspace(kinds, dt, 3, 2, m, frame_start=3, frame_end=67, frame_jump=2, **kw)
        assert part[2] == 32 and torch.equal(part[0], z[3:67:2]) and torch.equal(part[1], zp[3:67:2])           # sub-ranges
        assert torch.equal(snaps.simulate_subspace(kinds, dt, 3, 2, m, chunk_frames=16, **kw)[0], z)            # chunk width
        every = snaps.simulate_subspace(kinds, dt, 3, 2, m, record_every=2, **kw)
        assert every[3][1] == [2] and torch.equal(every[3][0][0], rec[1])
        # T1 steps continued by T2 (pins: shift_start raised by the steps taken)
        for t1 in (1, 2):
            a = snaps.simulate_subspace(kinds, dt, t1, 2, m, **kw)
            assert torch.equal(a[0], rec[t1 - 1])
            P2 = None if P is None else dict(P, shift_start=t1)
            b = snaps.simulate_subspace(kinds, dt, 3 - t1, 2, m, state=(a[0], a[1]), gravity=g, pins=P2)
            assert torch.equal(b[0], z) and torch.equal(b[1], zp)
        # the start is the projection of the frames
        z0 = snaps.subspace_coordinates("train")
        one = snaps.simulate_subspace(kinds, dt, 1, 2, m, **kw)
        assert torch.equal(one[1], z0)


def test_a_rollout_after_one_of_another_shape_equals_a_fresh_context():
    import torch
    s = zc.z_case("tris_blocks", 4)
    c = s["rf"]
    frames = np.array(s["frames"])
    kinds = [hyper_spec(c, 3)]
    fresh = _fixture_snaps(frames[:20], 4).simulate_subspace(kinds, s["dt"], 2, 2, s["masses"])[0]
    b = zc.z_case("tets_deim", 8)
    big = _fixture_snaps(np.array(b["frames"])[:70], 8)
    big.simulate_subspace([hyper_spec(b["rf"], 17)], b["dt"], 2, 3, b["masses"], pins=zc.pins_dict("fixed", b["rf"].g["rest"]))
    small = _snaps(frames[:20], svd_basis(frames[:20]), 4, frames[0], engine=big._engine)
    assert small._engine is big._engine
    assert torch.equal(small.simulate_subspace(kinds, s["dt"], 2, 2, s["masses"])[0], fresh)


# ------------------------------------------------------------------ 7. refusals and error codes
def test_refusals_and_error_codes():
    import torch
    from animsnapbases_amd import _lib
    s = zc.z_case("tris_blocks", 4)
    c = s["rf"]
    frames = np.array(s["frames"])
    kinds = [hyper_spec(c, 3)]
    p = _lib.ptr
    # without a subspace: ASB_ERR_ARG from every entry
    bare = _snaps(frames)
    bare.global_solve_setup([_plain(kinds[0])], s["dt"], s["masses"])
    e0 = bare._engine
    buf = torch.zeros((frames.shape[0], 4, 3), dtype=torch.float64, device="cuda:%d" % e0.device_id)
    big = torch.zeros((frames.shape[0], frames.shape[1], 3), dtype=torch.float64, device=buf.device)
    diag, acc, tv = np.ones(frames.shape[1]), np.zeros(3), np.arange(3, dtype=np.int64)
    import ctypes
    V = ctypes.c_void_p
    assert e0.lib.asb_zroll_operator(e0.h) == _lib.ERR_ARG and b"no position subspace" in e0.lib.asb_last_error(e0.h)
    assert e0.lib.asb_zroll_begin(e0.h, 0, 0, 5, 1, None, 0, 1.0, p(diag), 1, p(acc), 3, p(tv), None, None) == _lib.ERR_ARG
    assert e0.lib.asb_gsub_coordinates(e0.h, 0, 0, 5, 1, None, 0, 1.0, None, 0, V(buf.data_ptr())) == _lib.ERR_ARG
    assert e0.lib.asb_gsub_expand(e0.h, V(buf.data_ptr()), 5, V(big.data_ptr())) == _lib.ERR_ARG
    assert e0.lib.asb_zroll_steps(e0.h, 1, 1, 0, 0, None) == _lib.ERR_ARG and e0.lib.asb_zroll_state(e0.h, V(buf.data_ptr()), V(buf.data_ptr())) == _lib.ERR_ARG
    assert e0.lib.asb_zroll_slot(e0.h, 1.0, 1.0) == _lib.ERR_ARG and e0.lib.asb_zroll_pins(e0.h, 0) == _lib.ERR_ARG
    # counts before pointers: nothing behind them is read
    snaps = _fixture_snaps(frames, 4)
    z, zp, F = snaps.simulate_subspace(kinds, s["dt"], 2, 2, s["masses"])
    eng = snaps._engine
    assert eng.lib.asb_zroll_begin(eng.h, 0, 0, 5, 1, None, 0, 1.0, p(diag), 1, p(acc), 0, p(tv), None, None) == _lib.ERR_ARG
    assert eng.lib.asb_gsub_expand(eng.h, V(1), 0, V(1)) == _lib.ERR_ARG
    assert eng.lib.asb_test_zroll_affine(eng.h, 0, 1, 1, p(tv), p(diag), p(diag), p(diag), 0, p(diag)) == _lib.ERR_ARG
    assert eng.lib.asb_zroll_begin(eng.h, 0, 0, 5, 1, None, 0, 1.0, p(diag), 2, p(acc), 3, p(tv), None, None) == _lib.ERR_ARG and b"mode" in eng.lib.asb_last_error(eng.h)
    for bad in (np.array([2, 1, 5], dtype=np.int64), np.array([0, 1, frames.shape[1]], dtype=np.int64)):
        assert eng.lib.asb_zroll_begin(eng.h, 0, 0, 5, 1, None, 0, 1.0, p(diag), 1, p(acc), 3, p(bad), None, None) == _lib.ERR_ARG
        assert b"ascending" in eng.lib.asb_last_error(eng.h)
    assert eng.lib.asb_zroll_begin(eng.h, 0, 0, 5, 1, None, 0, 1.0, p(diag), 1, p(acc), 3, p(tv), V(buf.data_ptr()), None) == _lib.ERR_ARG
    # a failed begin leaves no roll-out; steps without a kind
    assert eng.lib.asb_zroll_steps(eng.h, 1, 1, 0, 0, None) == _lib.ERR_ARG and b"no roll-out begun" in eng.lib.asb_last_error(eng.h)
    eng.zroll_begin(0, 0, 5, 1, None, False, snaps.pre_scale_factor, diag, 1, acc, tv)
    assert eng.lib.asb_zroll_steps(eng.h, 1, 1, 0, 0, None) == _lib.ERR_ARG
    for args in ((0, 1, 0, 0, None), (1, 0, 0, 0, None), (1, 1, -1, 0, None), (1, 1, 0, 1, None)):
        assert eng.lib.asb_zroll_steps(eng.h, *args) == _lib.ERR_ARG
    assert eng.lib.asb_zroll_pins(eng.h, 0) == _lib.ERR_ARG and b"no pins" in eng.lib.asb_last_error(eng.h)
    # a set-up between asb_zroll_operator and the steps: the stale operator is refused, not used
    calls = {}
    real_steps = eng.zroll_steps

    def steps_after_a_setup(*a, **k):
        A = snaps.global_matrix
        Qt, origin = snaps._subspace_solver()
        eng.gsub_setup(A, Qt, np.ascontiguousarray(frames[0]))
        calls["n"] = calls.get("n", 0) + 1
        return real_steps(*a, **k)
    eng.zroll_steps = steps_after_a_setup
    try:
        with pytest.raises(RuntimeError, match="changed since asb_zroll_begin|stale"):
            snaps.simulate_subspace(kinds, s["dt"], 2, 2, s["masses"])
    finally:
        del eng.zroll_steps
    assert calls["n"] == 1
    # ... and with the roll-out begun after the new set-up, only the operator is stale
    eng.zroll_begin(0, 0, 5, 1, None, False, snaps.pre_scale_factor, diag, 1, acc, np.arange(frames.shape[1], dtype=np.int64))
    assert eng.lib.asb_zroll_slot(eng.h, 1.0, 1.0) == _lib.ERR_ARG                           # (no element set-up in the touched numbering)
    again = snaps.simulate_subspace(kinds, s["dt"], 2, 2, s["masses"])
    assert torch.equal(again[0], z) and torch.equal(again[1], zp)                             # the engine recovers: same bits
    eng.gsub_setup(snaps.global_matrix, snaps._subspace_solver()[0], np.ascontiguousarray(frames[0]))
    eng.zroll_begin(0, 0, frames.shape[0], 1, None, False, snaps.pre_scale_factor, s["masses"] / s["dt"] ** 2, 1, acc, np.arange(frames.shape[1], dtype=np.int64))
    from animsnapbases_amd import projections as proj
    op = zc.operator(s, 3)
    eng.cproj_setup(proj.touched_setup(proj.subset_setup(s["kinds"][0][0], op.elements), frames.shape[1])[1])
    eng.rforce_solver(op.H, op.local_rows)
    eng.zroll_slot(1.0, 1.0)
    assert eng.lib.asb_zroll_steps(eng.h, 1, 1, 0, 0, None) == _lib.ERR_ARG and b"stale" in eng.lib.asb_last_error(eng.h)
    eng.zroll_operator()
    assert eng.lib.asb_zroll_steps(eng.h, 1, 1, 0, 0, None) == 0
    # a row of the shift beyond T_s: before the device is touched (ValueError), and at the C layer
    P = dict(vertices=[0, 3], wi=1.0, shift=np.zeros((frames.shape[0] + 1, 3)))
    with pytest.raises(ValueError, match="row %d of shift is needed" % (frames.shape[0] + 1)):
        snaps.simulate_subspace(kinds, s["dt"], 3, 2, s["masses"], pins=P)
    snaps.simulate_subspace(kinds, s["dt"], 2, 2, s["masses"], pins=P)
    assert eng.lib.asb_zroll_steps(eng.h, 1, 1, 0, 0, None) == _lib.ERR_ARG and b"row" in eng.lib.asb_last_error(eng.h)
    # state on the wrong device / shape: ValueError
    with pytest.raises(ValueError, match="state"):
        snaps.simulate_subspace(kinds, s["dt"], 2, 2, s["masses"], state=(z[:5], zp[:5]))
