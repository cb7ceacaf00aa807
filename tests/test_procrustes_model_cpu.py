"""CPU: the longdouble model of the alignment call (tests/procrustes_model.py) against the oracle's align_frames -- NumPy float64,
LAPACK's SVD -- wherever the oracle's answer is determined: full-rank frames (generic, mirrored, thin, far from the origin, with and
without `rigid`), and flat frames whenever LAPACK's free sign makes det(U V^T) positive.  The oracle's T lies within the model's
own float64 bound dT (the bar of the 3 x 3 solve is 8 x LAPACK's measured error, so LAPACK is inside it) and its float32 frames
within dx plus one float32 rounding.  The model's rotations stay orthogonal and proper at longdouble precision on every kind of
frame, flat ones included.
"""
import numpy as np
import pytest

import procrustes_model as pm
from oracle import asb_oracle as orc

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)

FULL_RANK = {
    "generic_50": lambda: pm.generic_frames(50, 3, 11),
    "generic_4": lambda: pm.generic_frames(4, 3, 12),
    "generic_257": lambda: pm.generic_frames(257, 3, 13),
    "mirrored_60": lambda: pm.generic_frames(60, 3, 14, mirror_frame=1),
    "far_100": lambda: pm.generic_frames(100, 3, 15, offset=1e6),
    "thin_1e-2": lambda: pm.sheet_frames(50, 3, 1e-2, 16)[0],
    "thin_1e-4": lambda: pm.sheet_frames(300, 3, 1e-4, 17)[0],
}


@pytest.mark.parametrize("rigid", [True, False])
@pytest.mark.parametrize("name", sorted(FULL_RANK))
def test_model_matches_the_oracle_on_full_rank_frames(name, rigid):
    frames = FULL_RANK[name]()
    model = pm.align(frames, rigid)
    al, T = orc.align_frames(frames, rigid)
    assert al.dtype == np.float32
    worst_T = worst_x = 0.0
    for f, rec in enumerate(model):
        assert rec["kind"] == "full", (name, f, rec["kind"])
        errT = np.abs(T[f].astype(LD) - rec["T"])
        assert (errT <= rec["dT"]).all(), (name, f, errT, rec["dT"])
        errx = np.abs(al[f].astype(LD) - rec["aligned"])
        bx = rec["dx"] + 2.0 ** -24 * np.abs(rec["aligned"])
        assert (errx <= bx).all(), (name, f, float((errx / bx).max()))
        worst_T = max(worst_T, float((errT[:3] / np.maximum(rec["dT"][:3], 1e-300)).max()))
        worst_x = max(worst_x, float((errx / bx).max()))
        if name.startswith("mirrored") and f == 1:
            assert np.linalg.det(rec["R"].astype(np.float64)) > 0 and np.linalg.det(rec["M"].astype(np.float64)) < 0
    print("%s rigid=%d: oracle T at %.3g of the bound, frames at %.3g" % (name, rigid, worst_T, worst_x))


@pytest.mark.parametrize("thickness,N,tilt", [(0.0, 50, False), (0.0, 300, True), (1e-8, 50, False), (1e-8, 300, False)])
def test_model_takes_the_proper_rotation_on_flat_frames(thickness, N, tilt):
    frames, A, d_rms = pm.sheet_frames(N, 4, thickness, 21 + N, tilt=tilt)
    model = pm.align(frames)
    agree = 0
    for f, rec in enumerate(model):
        assert rec["kind"] == "rank2", (f, rec["kind"], rec["s"])
        R = rec["R"]
        assert np.abs(R.T @ R - np.eye(3, dtype=LD)).max() <= 16 * EPS_LD
        assert abs(np.linalg.det(R.astype(np.float64)) - 1.0) <= 1e-14
        # the frame really lands on frame 0: root-mean-square distance at most that of the deformation it was built with
        rms = float(np.sqrt(((rec["aligned"] - frames[0].astype(LD)) ** 2).sum(axis=1).mean()))
        assert rms <= d_rms[f] + 1e-15, (f, rms, d_rms[f])
        # the reference's rule gives the same rotation whenever LAPACK's sign comes out positive
        U, _, Vt = np.linalg.svd(rec["M"].astype(np.float64))
        if np.linalg.det(U @ Vt) > 0:
            assert np.abs(U @ Vt - R.astype(np.float64)).max() <= float(rec["dR"]), f
            agree += 1
    print("flat thickness %g N %d: LAPACK's sign positive on %d of %d frames" % (thickness, N, agree, len(model)))


def test_model_on_degenerate_point_counts():
    one, two, three = (pm.align(pm.generic_frames(n, 3, 30 + n)) for n in (1, 2, 3))
    for rec in one:
        assert rec["kind"] == "rank0" and (rec["T"][:3, :3] == np.eye(3)).all()
    x = pm.generic_frames(1, 3, 31).astype(LD)
    for f, rec in enumerate(one):                   # the one vertex lands on frame 0's
        assert (np.abs(rec["aligned"] - x[0]) <= 4 * EPS_LD * (np.abs(x[f]) + np.abs(x[0]))).all()
    assert [rec["kind"] for rec in two] == ["rank1"] * 3 and all(rec["T"] is None for rec in two)
    assert [rec["kind"] for rec in three] == ["rank2"] * 3
