"""GPU (-m gpu): ``subspace_rollout_errors`` and ``subspace_distance`` (animsnapbases_amd/dynamics.py) on the
fixtures of tests/zroll_cases.py -- "tris_blocks", "tets_deim" and the pinned "tris_blocks" with fixed pins -- with r in {4, 8},
K = 3 iterations, T = 3 steps, ``record_every=1``, ``frame_jump=3``.  Every measured err / bound is printed.

The sweep against the sweep MADE BY HAND from public calls: ``simulate_frames`` with records, per r ``set_global_solver("subspace")``
and ``simulate_subspace`` with records, ``subspace_expand`` of every record, and the reference's three metrics of the two
(F', N, 3) tensors formed on the host in longdouble.  The roll-outs are the same calls, so the tensors are the same bits and only
the metrics' arithmetic differs:
  max      max |e| / max a with e = fl(a - q~): formed in f64 from the same tensors, it equals the device's exactly.
  fro      the device's sums of N F' non-negative terms per axis carry at most N F' u each (u = eps / 2), the rounding of e itself
           2 u more, the host's sum of the three axes 2 u, the square root halves the relative error and rounds once:
           (N F' + 16) eps / 2 = (N F' + 16) u covers N F' u / 2 + 3 u.
  rel_*    the quotient of two such square roots, each N F' u / 2 + 2 u, and one division: N F' u + 5 u <= (N F' + 16) u.
Both baselines, the slab solver, a constant force on a vertex subset, the selected solver on every way out, ``subspace_distance``.
Every test fails on the parent commit, where the methods do not exist.

Largest err / bound measured on an MI355X: tris_blocks 1.2e-3, tets_deim 1.8e-3, pinned 5.7e-4, under "slab" 2.5e-3, forced 6.9e-4, per
frame 1.8e-2; the baselines differ by 1.0e11 bounds, the forced roll-outs moved by 2.8e11 / 8.0e10 bounds (also in DESIGN.md 3.23)."""
import numpy as np
import pytest

import pins_cases as pins
import zroll_cases as zc
from gsub_model import EPS, LD, svd_basis
from test_gpu_gsub import _snaps
from test_gpu_hyper import _spec as hyper_spec

pytestmark = pytest.mark.gpu

RS = [4, 8]
K, T = 3, 3
CASES = [("tris_blocks", None, 8), ("tets_deim", None, 17), ("tris_blocks", "fixed", 8)]


def _case(fixture, pn, m):
    """(snapshots with no solver selected, the case, kinds, basis, origin, the keyword arguments both roll-outs take)."""
    s = zc.z_case(fixture, 4, pn)
    frames = np.array(s["frames"])
    kw = dict(masses=s["masses"], frame_jump=3)
    if pn is not None:
        kw.update(pins=s["pins_dict"], gravity=pins.G)
    return _snaps(frames), s, [hyper_spec(s["rf"], m)], svd_basis(frames), frames[0].copy(), kw


def _plain(spec):
    return {k: v for k, v in spec.items() if k not in ("basis", "num_components", "reduction")}


def _host_metrics(a, q):
    """The reference's three metrics of (a, q) in longdouble; max in f64, as the device forms it."""
    e = a.astype(LD) - q.astype(LD)
    s, nrm = (e ** 2).sum(axis=(0, 1)), (a.astype(LD) ** 2).sum(axis=(0, 1))
    return [np.sqrt(s.sum())] + [float(np.abs(a - q).max() / a.max())] + [np.sqrt(s[d]) / np.sqrt(nrm[d]) for d in range(3)]


def _by_hand(snaps, s, kinds, basis, origin, rs, baseline, kw, solver=("inverse", {})):
    """The sweep from public calls: ((5, len(rs), T) longdouble, the baseline's records, the z records of the last r)."""
    snaps.set_global_solver(solver[0], **solver[1])
    if baseline == "reduced":
        full = snaps.simulate_frames(kinds, s["dt"], T, K, hyper="touched", record_every=1, **kw)[3][0]
    else:
        full = snaps.simulate_frames([_plain(k) for k in kinds], s["dt"], T, K, record_every=1, **kw)[3][0]
    out = np.zeros((5, len(rs), T), dtype=LD)
    zrec = None
    for i, r in enumerate(rs):
        snaps.set_global_solver("subspace", basis=basis, num_components=r, origin=origin)
        zrec = snaps.simulate_subspace(kinds, s["dt"], T, K, record_every=1, **kw)[3][0]
        for j in range(T):
            out[:, i, j] = _host_metrics(full[j].cpu().numpy(), snaps.subspace_expand(zrec[j]).cpu().numpy())
    return out, full, zrec


def _compare(tag, got, want, n_terms):
    """The sweep's five arrays against the hand-made ones: max exact, the others within (N F' + 16) eps / 2, relative."""
    assert got[5] == list(range(1, T + 1))
    for a in got[:5]:
        assert a.shape == want.shape[1:] and np.isfinite(a).all()
    assert np.array_equal(got[1], want[1].astype(np.float64)), (tag, got[1], want[1])
    bound = (n_terms + 16) * EPS / 2.0
    worst = 0.0
    for k in (0, 2, 3, 4):
        ratio = (np.abs(got[k] - want[k]) / (bound * want[k])).astype(np.float64)
        worst = max(worst, float(ratio.max()))
    print("%s: largest err / bound %.3g (bound %.3g relative)" % (tag, worst, bound))
    assert worst <= 1.0
    return bound


@pytest.mark.parametrize("fixture,pn,m", CASES)
def test_the_sweep_equals_the_sweep_made_by_hand(fixture, pn, m):
    import torch
    snaps, s, kinds, basis, origin, kw = _case(fixture, pn, m)
    N, nF = snaps.nVerts, len(zc.SEL)
    got = snaps.subspace_rollout_errors(kinds, basis, RS, s["dt"], T, K, origin=origin, **kw)
    assert not hasattr(snaps, "_global_solver")                                               # none was selected: none afterwards
    want, full, zrec = _by_hand(snaps, s, kinds, basis, origin, RS, "reduced", kw)
    _compare("%s %s" % (fixture, pn), got, want, N * nF)
    assert tuple(full.shape) == (T, nF, N, 3)
    assert (got[0] > 0).all()
    # subspace_distance (the last r is on the device): one cell of the sweep, bit for bit
    j = T - 1
    cell = snaps.subspace_distance(full[j], zrec[j])
    assert cell == tuple(float(got[k][-1, j]) for k in range(5))
    out = snaps.subspace_distance(full[j], zrec[j], per_frame=True)
    assert out[:5] == cell and out[5].shape == (nF,) and np.isfinite(out[5]).all()
    a, q = full[j].cpu().numpy(), snaps.subspace_expand(zrec[j]).cpu().numpy()
    e2, a2 = ((a.astype(LD) - q.astype(LD)) ** 2).sum(axis=(1, 2)), (a.astype(LD) ** 2).sum(axis=(1, 2))
    ratio = (np.abs(out[5] - np.sqrt(e2) / np.sqrt(a2)) / ((3 * N + 16) * EPS * np.sqrt(e2) / np.sqrt(a2))).astype(np.float64)
    print("%s %s per frame: largest err / bound %.3g" % (fixture, pn, float(ratio.max())))
    assert (ratio <= 1.0).all()
    # on the expansion itself: exact zeros
    zero = snaps.subspace_distance(snaps.subspace_expand(zrec[j]), zrec[j], per_frame=True)
    assert zero[:5] == (0.0, 0.0, 0.0, 0.0, 0.0) and (zero[5] == 0.0).all()
    # refusals of subspace_distance on real tensors: F' and the device
    for bx, bz in ((full[j][:5], zrec[j]), (full[j], zrec[j][:, :3]), (full[j].cpu(), zrec[j]), (full[j], zrec[j].float())):
        with pytest.raises(ValueError, match="subspace_distance"):
            snaps.subspace_distance(bx, bz)
    assert torch.equal(snaps.subspace_expand(zrec[j]), torch.tensor(q, device=zrec.device))


def test_both_baselines():
    """Against the unreduced simulator the drift contains the DEIM reduction's (m = 3 of tris_blocks): the two baselines differ
    by far more than the bounds, and each equals its sweep made by hand."""
    snaps, s, kinds, basis, origin, kw = _case("tris_blocks", None, 3)
    N, nF = snaps.nVerts, len(zc.SEL)
    red = snaps.subspace_rollout_errors(kinds, basis, RS, s["dt"], T, K, origin=origin, baseline="reduced", **kw)
    full = snaps.subspace_rollout_errors(kinds, basis, RS, s["dt"], T, K, origin=origin, baseline="full", **kw)
    bound = _compare("tris_blocks m = 3, baseline reduced", red, _by_hand(snaps, s, kinds, basis, origin, RS, "reduced", kw)[0], N * nF)
    _compare("tris_blocks m = 3, baseline full", full, _by_hand(snaps, s, kinds, basis, origin, RS, "full", kw)[0], N * nF)
    snaps.set_global_solver("inverse")
    gap = np.abs(full[0] - red[0]) / (bound * np.maximum(full[0], red[0]))
    print("baselines: |fro_full - fro_reduced| / bound at least %.3g" % float(gap.min()))
    assert (gap > 1e6).all()


def test_under_the_slab_solver():
    snaps, s, kinds, basis, origin, kw = _case("tets_deim", None, 17)
    snaps.set_global_solver("slab", slab_target=6)
    got = snaps.subspace_rollout_errors(kinds, basis, RS, s["dt"], T, K, origin=origin, **kw)
    assert snaps._global_solver == ("slab", 6) and snaps._global_subspace is None
    want = _by_hand(snaps, s, kinds, basis, origin, RS, "reduced", kw, ("slab", dict(slab_target=6)))[0]
    _compare("tets_deim under slab", got, want, snaps.nVerts * len(zc.SEL))


def test_a_constant_force_on_a_vertex_subset():
    snaps, s, kinds, basis, origin, kw = _case("tris_blocks", None, 8)
    N, nF = snaps.nVerts, len(zc.SEL)
    v = np.array([1, 7, 20, 33], dtype=np.int64)
    extent = float(np.ptp(np.array(s["frames"])[0], axis=0).max())
    force = np.zeros((v.size, 3))
    force[:, 1] = -0.05 * extent * s["masses"][v] / s["dt"] ** 2                               # dt^2 f / m = 5 % of the mesh's extent per step
    forced = dict(kw, forces=dict(force=force, vertices=v))
    got = snaps.subspace_rollout_errors(kinds, basis, RS, s["dt"], T, K, origin=origin, **forced)
    want, full, zrec = _by_hand(snaps, s, kinds, basis, origin, RS, "reduced", forced)
    bound = _compare("tris_blocks forced", got, want, N * nF)
    q = snaps.subspace_expand(zrec[-1]).cpu().numpy()
    _, free_full, free_z = _by_hand(snaps, s, kinds, basis, origin, RS, "reduced", kw)
    free_q = snaps.subspace_expand(free_z[-1]).cpu().numpy()
    a, free_a = full[-1].cpu().numpy(), free_full[-1].cpu().numpy()
    for name, x, y in (("full", a, free_a), ("z", q, free_q)):
        moved = float(np.abs(x - y).max()) / (bound * float(np.abs(y).max()))
        print("forced %s roll-out moved by %.3g bounds" % (name, moved))
        assert moved > 1e6
    snaps.set_global_solver("inverse")


def test_the_selected_solver_is_restored():
    snaps, s, kinds, basis, origin, kw = _case("tets_deim", "moving", 17)
    snaps.set_global_solver("slab")
    before = (snaps._global_solver, snaps._global_subspace)
    short = dict(s["pins_dict"], shift=s["pins_dict"]["shift"][:zc.SEL[-1] + T - 1])          # the last step's row is missing
    with pytest.raises(ValueError, match="subspace_rollout_errors: pins: row %d of shift is needed" % (zc.SEL[-1] + T - 1)):
        snaps.subspace_rollout_errors(kinds, basis, RS, s["dt"], T, K, origin=origin, **dict(kw, pins=short))
    assert (snaps._global_solver, snaps._global_subspace) == before
    # an engine's refusal from inside the second roll-out in z
    eng = snaps._engine
    real, count = eng.zroll_steps, {"n": 0}

    def second(*a, **k):
        count["n"] += 1
        if count["n"] == 2:
            raise ValueError("inside")
        return real(*a, **k)
    eng.zroll_steps = second
    try:
        with pytest.raises(ValueError, match="inside"):
            snaps.subspace_rollout_errors(kinds, basis, RS, s["dt"], T, K, origin=origin, **kw)
    finally:
        del eng.zroll_steps
    assert count["n"] == 2 and (snaps._global_solver, snaps._global_subspace) == before
    got = snaps.subspace_rollout_errors(kinds, basis, RS, s["dt"], T, K, origin=origin, **kw)      # and the object still works
    assert (snaps._global_solver, snaps._global_subspace) == before and np.isfinite(got[0]).all()
    with pytest.raises(ValueError, match="set_global_solver\\('subspace'\\) is in force"):
        snaps.set_global_solver("subspace", basis=basis, num_components=4, origin=origin)
        snaps.subspace_rollout_errors(kinds, basis, RS, s["dt"], T, K, origin=origin, **kw)
