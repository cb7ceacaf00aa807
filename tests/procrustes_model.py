"""numpy.longdouble model of the whole alignment call (asb_align_frames, csrc/asb_ingest.hip) and the forward bounds of its float64
arithmetic, shared by tests/test_procrustes_model_cpu.py and tests/test_gpu_procrustes.py.  Not a test module.

Per frame f, as utils/process.py:210-234 of the reference: t0 = centroid(frame f), t1 = centroid(frame 0),
M = (frame 0 - t1)^T (frame f - t0), R from the SVD of M, T = [R | t1 - R t0] (R replaced by I in the rotation block when
`rigid` is off, the translation still from R), aligned = frame f R^T + t.  Sums and products in longdouble (64-bit mantissa), the
3 x 3 SVD in mpmath at 60 digits on the longdouble M, with the rule of tests/procrustes_cases.py by the singular values:
full rank -> the reference's U V^T (x -1 where det < 0); rank 2 -> the proper rotation; rank 1 -> no unique rotation (R is None);
M = 0 -> I.  A frame whose M lies in the band between full rank and deficient is an error of the test's inputs.

Bounds (eps = 2^-52, twice the unit round-off, so every "n roundings" below is counted double):
  centroid    dt_a  <= (N + 1) eps sum_v |x_va| / N                      N - 1 additions in any tree order and the division
  M           dM_ab <= (N + 3) eps sum_v |q_va| |p_vb| + N dt1_a dt0_b   two subtractions, the product, N - 1 additions per
              term; the centroid errors enter in second order only, because sum_v p_v = sum_v q_v = 0 for the exact centroids
  R           dR    <= b eps s1 / (s2 + s3)  +  2 |dM|_F / (s2 + s3)     the solve's own bar (procrustes_cases.bounds, rot) plus
              the perturbation bound of the real orthogonal polar factor (R.-C. Li, SIAM J. Matrix Anal. Appl. 16 (1995):
              |dQ|_F <= 2 |dA|_F / (s_n + s_(n-1))).  For rank 2 the device's R is the polar factor of its M with the sign of
              s3 made positive, a matrix within 2 s3' of its M, s3' <= s3 + |dM|_F: |dM|_F is replaced by 3 |dM|_F + 4 s3.
  t           dt_a  <= dt1_a + sum_b (dR |t0_b| + |R_ab| dt0_b) + 4 eps (|t1_a| + sum_b |R_ab| |t0_b|)
  aligned     dx_a  <= sum_b dR |x_b| + dt_a + 4 eps (sum_b |R_ab| |x_b| + |t_a|)
"""
import mpmath as mp
import numpy as np

import procrustes_cases as pc

LD = np.longdouble
EPS = pc.EPS


def _to_mp(x):
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - LD(hi)))


def _to_ld(x):
    hi = float(x)
    return LD(hi) + LD(float(x - mp.mpf(hi)))


def rotation(M):
    """M (3 x 3 longdouble) -> dict(kind, s (floats), R (3 x 3 longdouble or None))"""
    M = np.asarray(M, dtype=LD)
    if not M.any():
        return dict(kind="rank0", s=np.zeros(3), R=np.eye(3, dtype=LD))
    with mp.workdps(pc.DPS):
        A = mp.matrix([[_to_mp(x) for x in row] for row in M])
        U, S, Vt = mp.svd_r(A)
        s = [S[i] for i in range(3)]
        kind = pc.kind_of(s)
        assert kind != "band", "s = %r: between full rank and deficient" % ([float(x) for x in s],)
        R = None
        if kind != "rank1":
            Rm = pc.rule_rotation(U, Vt, proper=(kind == "rank2"))
            R = np.array([[_to_ld(Rm[i, j]) for j in range(3)] for i in range(3)], dtype=LD)
        return dict(kind=kind, s=np.array([float(x) for x in s]), R=R)


def cross_covariance(frame, frame0):
    """-> t0, t1, M in longdouble and the float64 error bounds dt0, dt1 (3), dM (3 x 3) of the device's sums"""
    p, q = np.asarray(frame, dtype=LD), np.asarray(frame0, dtype=LD)
    N = p.shape[0]
    t0, t1 = p.sum(axis=0) / N, q.sum(axis=0) / N
    dt0, dt1 = (N + 1) * EPS * np.abs(p).sum(axis=0) / N, (N + 1) * EPS * np.abs(q).sum(axis=0) / N
    pc_, qc = p - t0, q - t1
    M = qc.T @ pc_
    dM = (N + 3) * EPS * (np.abs(qc).T @ np.abs(pc_)) + N * np.outer(dt1, dt0)
    return t0, t1, M, dt0, dt1, dM


# the 3 x 3 solve's bar on R by the kind of M: the loosest of the full-rank families that point sets produce, and rank 2's
B_ROT = {"full": max(pc.bounds(fam)["rot"] for fam in ("generic", "mirrored", "thin")), "rank2": pc.bounds("rank2")["rot"]}


def align(frames, rigid=True):
    """frames (F, N, 3) float64 -> list over the frames of dict(kind, s, R, T (4 x 4 longdouble), aligned (N, 3 longdouble),
    M, dM, t0, t1, dt0, dt1, dR (scalar bound on every entry of R), dT (4 x 4 bound), dx (N, 3 bound on the aligned frame));
    T, aligned and the bounds are None for a rank-1 frame."""
    frames = np.asarray(frames, dtype=np.float64)
    out = []
    for f in range(frames.shape[0]):
        t0, t1, M, dt0, dt1, dM = cross_covariance(frames[f], frames[0])
        rot = rotation(M)
        rec = dict(rot, M=M, dM=dM, t0=t0, t1=t1, dt0=dt0, dt1=dt1, T=None, aligned=None, dR=None, dT=None, dx=None)
        R = rot["R"]
        if R is not None:
            s = rot["s"]
            dMF = float(np.sqrt((dM * dM).sum()))
            if rot["kind"] == "rank0":
                dR = 0.0                                    # the device's M is zero as well: N = 1, or every point on the centroid
            else:
                if rot["kind"] == "rank2":
                    dMF = 3 * dMF + 4 * s[2]
                dR = (B_ROT[rot["kind"]] * EPS * s[0] + 2 * dMF) / (s[1] + s[2])
            aR = np.abs(R)
            t = t1 - R @ t0
            dt = dt1 + dR * np.abs(t0).sum() + aR @ dt0 + 4 * EPS * (np.abs(t1) + aR @ np.abs(t0))
            T = np.eye(4, dtype=LD)
            dT = np.zeros((4, 4), dtype=LD)
            if rigid:
                T[:3, :3] = R
                dT[:3, :3] = dR
            T[:3, 3] = t
            dT[:3, 3] = dt
            x = frames[f].astype(LD)
            L, aL, dL = T[:3, :3], np.abs(T[:3, :3]), (dR if rigid else 0.0)
            rec.update(T=T, dT=dT, dR=dR, aligned=x @ L.T + t,
                       dx=dL * np.abs(x).sum(axis=1, keepdims=True) + dt + 4 * EPS * (np.abs(x) @ aL.T + np.abs(t)))
        out.append(rec)
    return out


# --------------------------------------------------------------------------------------
# seeded inputs shared by the CPU and the GPU tests
# --------------------------------------------------------------------------------------
def rotation_matrix(rng):
    """a random proper rotation"""
    Q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    if np.linalg.det(Q) < 0:
        Q[:, 0] *= -1
    return Q


def generic_frames(N, F, seed, noise=1e-3, offset=0.0, mirror_frame=None):
    """generic 3-D points in a 1 x 0.8 x 0.6 box; frame f > 0 = (frame 0 + noise) rotated properly and translated.  `offset`: every
    frame, frame 0 included, is moved by its own vector of that size.  `mirror_frame`: that frame is reflected through a plane
    before it is rotated."""
    rng = np.random.default_rng(seed)
    rest = rng.uniform(-0.5, 0.5, size=(N, 3)) * np.array([1.0, 0.8, 0.6])
    frames = [rest]
    for f in range(1, F):
        x = rest + noise * rng.uniform(-1, 1, size=rest.shape)
        if f == mirror_frame:
            n = rng.normal(size=3)
            n /= np.linalg.norm(n)
            x = x @ (np.eye(3) - 2 * np.outer(n, n)).T
        frames.append(x @ rotation_matrix(rng).T + rng.uniform(-2, 2, size=3))
    frames = np.array(frames)
    if offset:
        frames = frames + offset * rng.uniform(-1, 1, size=(F, 1, 3))
    return frames


def sheet_frames(N, F, thickness, seed, amp=1e-3, tilt=False):
    """a 1 x 1 sheet of z-extent `thickness` as frame 0 (in the plane z = 0, or tilted out of it); frame f > 0 = (frame 0 + d) rotated
    properly and translated, |d_x|, |d_y| <= amp, |d_z| <= amp thickness.  -> frames, the largest |d| a vertex can have, the
    root mean square of |d| per frame"""
    rng = np.random.default_rng(seed)
    rest = rng.uniform(-0.5, 0.5, size=(N, 3)) * np.array([1.0, 1.0, thickness])
    Q0 = rotation_matrix(rng) if tilt else np.eye(3)
    frames, rms = [rest @ Q0.T], [0.0]
    for f in range(1, F):
        d = amp * rng.uniform(-1, 1, size=rest.shape) * np.array([1.0, 1.0, thickness])
        rms.append(float(np.sqrt((d * d).sum(axis=1).mean())))
        frames.append((rest + d) @ (rotation_matrix(rng) @ Q0).T + rng.uniform(-2, 2, size=3))
    return np.array(frames), amp * float(np.sqrt(2.0 + thickness * thickness)), np.array(rms)
