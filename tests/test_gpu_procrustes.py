"""GPU (-m gpu): asb_align_frames (k_procrustes + k_apply_rbm, csrc/asb_ingest.hip) at small shapes against the longdouble model of
tests/procrustes_model.py, within the forward bounds derived there (the bar of the 3 x 3 solve from procrustes_cases.LAPACK_WORST,
plus N eps sum |term| for the centroids and M formed in float64, pushed through the conditioning 2 / (s2 + s3) of the polar factor).

  N edges        N = 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1000 (one wave, one block, the block's stride), F = 3.  N = 1 gives M = 0
                 (R = I exactly), N = 2 rank 1 (finite, orthogonal, proper, optimal; T maps centroid onto centroid), N = 3 rank 2.
  F = 1          T[0] is the identity and the frame comes back unchanged, both to the bound.
  flat and thin  a sheet of z-extent 0, 1e-8, 1e-4, 1e-2 as frame 0 (in a coordinate plane and tilted), N = 50 and 300; a flat frame 2
                 against a generic frame 0.  R^T R = I, det R = +1, and every aligned frame lies on frame 0: its root-mean-square
                 distance is at most that of the deformation d it was built with (the optimum does no worse than the true motion),
                 and no vertex is farther than 6 max|d| (the optimum differs from the true motion by a rigid field g with
                 rms(g) <= 2 rms(d), and on a square sheet max|g| <= 2.5 rms(g)).
  mirrored       one frame reflected through a plane, full rank: the reference's -U V^T, the oracle agrees within twice the bound.
  far away       every frame offset by its own vector of 1e6 x extent: the N eps sum |term| of the centroids dominates the bound.
  rigid = 0      rotation block the identity exactly, translation still t1 - R t0.
  grid stride    N = 1024 * 256 + 3, F = 2: every vertex equals the returned T applied to the input in longdouble within
                 4 eps (|T| |x| + |t|), and every vertex of frame 1 has moved.

Each test prints achieved / bound; the figures of one run are in tests/README.md.
"""
import numpy as np
import pytest

import procrustes_cases as pc
import procrustes_model as pm

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = pc.EPS
B_ORTH = max(pc.bounds(fam)["orth"] for fam in pc.LAPACK_WORST)          # |R^T R - I| <= B_ORTH eps on every kind of M
B_DET = 2 * B_ORTH             # det(R)^2 = det(I + E) = 1 + tr E + O(E^2): |det R - 1| <= 1.5 max|E| + O(E^2)


def _device(frames, rigid=True):
    from animsnapbases_amd import HipEngine
    e = HipEngine(0)
    try:
        return e.align_frames(frames, rigid)
    finally:
        e.close()


def _check_rotation(R, label):
    R = R.astype(LD)
    assert np.isfinite(R.astype(np.float64)).all(), label
    orth = float(np.abs(R.T @ R - np.eye(3, dtype=LD)).max())
    det = float(abs(R[0] @ np.cross(R[1], R[2]) - 1))
    assert orth <= B_ORTH * EPS, "%s: |R^T R - I| = %.3g eps" % (label, orth / EPS)
    assert det <= B_DET * EPS, "%s: |det R - 1| = %.3g eps" % (label, det / EPS)
    return orth / (B_ORTH * EPS), det / (B_DET * EPS)


def _check_against_model(label, frames, al, T, model, rigid=True):
    """T and the aligned frames within the model's bounds, frame by frame; prints the worst achieved / bound"""
    assert al.shape == frames.shape and T.shape == (frames.shape[0], 4, 4)
    wT = wx = wo = 0.0
    for f, rec in enumerate(model):
        assert rec["T"] is not None, (label, f, rec["kind"])
        assert (T[f, 3] == [0.0, 0.0, 0.0, 1.0]).all(), (label, f)
        errT = np.abs(T[f].astype(LD) - rec["T"])[:3]
        errx = np.abs(al[f].astype(LD) - rec["aligned"])
        rT, rx = float((errT / np.maximum(rec["dT"][:3], 1e-300)).max()), float((errx / rec["dx"]).max())
        assert (errT <= rec["dT"][:3]).all(), "%s frame %d (%s): T at %.3g of the bound\n%r" % (label, f, rec["kind"], rT, T[f])
        assert (errx <= rec["dx"]).all(), "%s frame %d (%s): aligned frame at %.3g of the bound" % (label, f, rec["kind"], rx)
        if rigid:
            wo = max(wo, *_check_rotation(T[f, :3, :3], "%s frame %d" % (label, f)))
        else:
            assert (T[f, :3, :3] == np.eye(3)).all(), (label, f)
        wT, wx = max(wT, rT), max(wx, rx)
    print("%s: T at %.3g of the bound, aligned frames at %.3g, orthogonality / det at %.3g" % (label, wT, wx, wo))


@pytest.mark.parametrize("N", [3, 4, 63, 64, 65, 255, 256, 257, 1000])
def test_vertex_counts_around_the_wave_and_the_block(N):
    frames = pm.generic_frames(N, 3, 100 + N)
    model = pm.align(frames)
    assert [rec["kind"] for rec in model] == (["rank2"] * 3 if N == 3 else ["full"] * 3)
    al, T = _device(frames)
    _check_against_model("N = %d" % N, frames, al, T, model)


def _check_centroid_mapping(label, frames, T, model):
    """T maps the centroid of each frame onto that of frame 0: T c = t1' + R (c - t0'), the primes being the device's centroids"""
    worst = 0.0
    for f, rec in enumerate(model):
        got = T[f, :3, :3].astype(LD) @ rec["t0"] + T[f, :3, 3].astype(LD)
        bound = rec["dt1"] + rec["dt0"].sum() + 8 * EPS * (np.abs(rec["t1"]) + np.abs(rec["t0"]).sum())
        err = np.abs(got - rec["t1"])
        assert (err <= bound).all(), (label, f, err, bound)
        worst = max(worst, float((err / bound).max()))
    return worst


def test_one_vertex_gives_the_identity_and_a_translation():
    frames = pm.generic_frames(1, 3, 101)
    model = pm.align(frames)
    assert [rec["kind"] for rec in model] == ["rank0"] * 3
    al, T = _device(frames)
    assert (T[:, :3, :3] == np.eye(3)).all()
    _check_against_model("N = 1", frames, al, T, model)
    print("N = 1: centroid mapping at %.3g of the bound" % _check_centroid_mapping("N = 1", frames, T, model))


def test_two_vertices_give_a_proper_optimal_rotation():
    """rank 1: no unique R; finite, orthogonal, proper, tr(R^T M) >= s1 (1 - b eps) up to the error of the device's M, and the
    segment of every frame lands on frame 0's to within the noise the frames were built with"""
    frames = pm.generic_frames(2, 3, 102)
    model = pm.align(frames)
    assert [rec["kind"] for rec in model] == ["rank1"] * 3
    al, T = _device(frames)
    b_opt = pc.bounds("rank1")["opt"]
    for f, rec in enumerate(model):
        assert (T[f, 3] == [0.0, 0.0, 0.0, 1.0]).all()
        o, d = _check_rotation(T[f, :3, :3], "N = 2 frame %d" % f)
        R, s1 = T[f, :3, :3].astype(LD), rec["s"][0]
        gap = s1 - float((R * rec["M"]).sum())                   # s1 - tr(R^T M)
        bound = (b_opt + B_ORTH) * EPS * s1 + 2 * float(rec["dM"].sum())       # |R_ab| <= 1 + B_ORTH eps, s1' >= s1 - |dM|_F
        assert gap <= bound, (f, gap, bound)
        print("N = 2 frame %d: orthogonality at %.3g, det at %.3g, optimality gap at %.3g of the bound" % (f, o, d, gap / bound))
        want = (frames[f].astype(LD) @ R.T + T[f, :3, 3].astype(LD))
        assert np.abs(al[f] - want).max() <= 4 * EPS * (np.abs(frames[f]).sum() + np.abs(T[f, :3, 3]).sum())
        assert np.abs(al[f] - frames[0]).max() <= 4e-3           # noise 1e-3 per coordinate on both end points
    print("N = 2: centroid mapping at %.3g of the bound" % _check_centroid_mapping("N = 2", frames, T, model))


def test_single_frame_is_returned_unchanged():
    frames = pm.generic_frames(65, 1, 103)
    model = pm.align(frames)
    al, T = _device(frames)
    _check_against_model("F = 1", frames, al, T, model)
    assert (np.abs(T[0] - np.eye(4))[:3] <= model[0]["dT"][:3]).all()
    assert (np.abs(al[0] - frames[0]) <= model[0]["dx"]).all()


def _check_lands_on_frame0(label, frames, al, A, d_rms, model):
    worst = 0.0
    for f in range(frames.shape[0]):
        dist = np.sqrt(((al[f] - frames[0]) ** 2).sum(axis=1))
        rms, slack = float(np.sqrt((dist ** 2).mean())), 2 * float(model[f]["dx"].max())          # the float64 error of al
        assert rms <= d_rms[f] + slack, (label, f, rms, d_rms[f])
        assert dist.max() <= 6 * A, (label, f, float(dist.max()), A)
        worst = max(worst, float(dist.max()))
    print("%s: farthest vertex %.3g from frame 0, deformation amplitude %.3g" % (label, worst, A))


SHEETS = [(t, N, False) for t in (0.0, 1e-8, 1e-4, 1e-2) for N in (50, 300)] + [(0.0, 50, True), (0.0, 300, True)]


@pytest.mark.parametrize("thickness,N,tilt", SHEETS)
def test_flat_and_thin_sheets(thickness, N, tilt):
    frames, A, d_rms = pm.sheet_frames(N, 4, thickness, 200 + N + int(tilt), tilt=tilt)
    model = pm.align(frames)
    assert [rec["kind"] for rec in model] == ["rank2" if thickness <= 1e-8 else "full"] * 4
    label = "sheet thickness %g N %d%s" % (thickness, N, " tilted" if tilt else "")
    al, T = _device(frames)
    _check_against_model(label, frames, al, T, model)
    _check_lands_on_frame0(label, frames, al, A, d_rms, model)


def test_flat_frame_against_a_generic_frame0():
    """M is deficient through the from side only"""
    frames = pm.generic_frames(50, 3, 104)
    flat = pm.sheet_frames(50, 2, 0.0, 105)[0]
    frames[2] = flat[1]
    model = pm.align(frames)
    assert [rec["kind"] for rec in model] == ["full", "full", "rank2"]
    al, T = _device(frames)
    _check_against_model("flat frame 2, generic frame 0", frames, al, T, model)


def test_mirrored_frame_follows_the_reference_rule():
    from oracle import asb_oracle as orc
    frames = pm.generic_frames(60, 3, 106, mirror_frame=1)
    model = pm.align(frames)
    assert [rec["kind"] for rec in model] == ["full"] * 3
    assert np.linalg.det(model[1]["M"].astype(np.float64)) < 0 < np.linalg.det(model[2]["M"].astype(np.float64))
    al, T = _device(frames)
    _check_against_model("mirrored frame 1", frames, al, T, model)
    # -U V^T of a reflection is a proper rotation that does NOT bring the frame onto frame 0: the reference's behaviour, kept
    assert np.abs(al[1] - frames[0]).max() > 0.1 and np.abs(al[2] - frames[0]).max() < 1e-2
    al_o, T_o = orc.align_frames(frames, True)
    for f, rec in enumerate(model):
        assert (np.abs(T[f] - T_o[f])[:3] <= 2 * rec["dT"][:3]).all(), f


def test_frames_far_from_the_origin():
    frames = pm.generic_frames(100, 3, 107, offset=1e6)
    model = pm.align(frames)
    al, T = _device(frames)
    _check_against_model("offset 1e6", frames, al, T, model)
    for f, rec in enumerate(model):
        # what the bound is made of here: the centroid term, not the 3 x 3 solve
        assert float(rec["dT"][:3, 3].max()) > 1e3 * pm.B_ROT["full"] * EPS
    assert np.abs(al - frames[0]).max() <= 1e-2                  # noise 1e-3, and 1e6 eps of cancellation


@pytest.mark.parametrize("which", ["generic", "sheet"])
def test_rigid_off_keeps_the_translation_of_the_rotation(which):
    frames = pm.generic_frames(257, 3, 108) if which == "generic" else pm.sheet_frames(50, 3, 1e-4, 109)[0]
    model = pm.align(frames, rigid=False)
    al, T = _device(frames, rigid=False)
    _check_against_model("rigid = 0, %s" % which, frames, al, T, model, rigid=False)
    R = pm.align(frames)[1]["R"]
    assert np.abs(R - np.eye(3)).max() > 0.1                     # the translation checked above is t1 - R t0 with a real R


def test_grid_stride_transforms_every_vertex_once():
    N = 1024 * 256 + 3
    frames = pm.generic_frames(N, 2, 110)
    al, T = _device(frames)
    worst = 0.0
    for f in range(2):
        x, L, t = frames[f].astype(LD), T[f, :3, :3].astype(LD), T[f, :3, 3].astype(LD)
        err = np.abs(al[f] - (x @ L.T + t))
        bound = 4 * EPS * (np.abs(x) @ np.abs(L).T + np.abs(t))
        bad = np.flatnonzero((err > bound).any(axis=1))
        assert bad.size == 0, "frame %d: %d vertices off, first %d" % (f, bad.size, bad[0])
        worst = max(worst, float((err / bound).max()))
    moved = np.abs(al[1] - frames[1]).max(axis=1)
    assert moved.min() > 0.1, "vertex %d of frame 1 was left where it was" % int(moved.argmin())
    print("grid stride: every vertex at %.3g of 4 eps (|T||x| + |t|)" % worst)
    _check_against_model("N = %d" % N, frames, al, T, pm.align(frames))
