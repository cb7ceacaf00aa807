"""TEST HELPER: NumPy restatement of the arithmetic of ``compute_accuracy`` (generate_figures/onMesh_accuracyMeasures.py:61-151)
on arrays.  The reference reads the frames of both animations from ``.off`` files and calls ``igl.per_vertex_normals``; here the
frames are (F, N, 3) arrays and the normals are written out from their definition (libigl 2.5.1's default for
``per_vertex_normals`` is area weighting: every corner of a triangle receives the triangle's un-normalised cross product, the
sums are normalised at the end).  libigl is not available to the tests, so that definition is not pinned against it."""
import numpy as np

# :95-98, spelling included
HEADER = ['numComponent', 'norm_error_min', 'norm_error_mean', 'norm_error_max', 'norm_error_sum',
          'angle_error_min', 'angle_error_mean', 'angle_error_max', 'angle_error_sum',
          "accum_norm_min", "accum_norm_meann", "accum_norm_max",
          "accum_angle_min", "accum_angle_mean", "accum_angle_max"]


def per_vertex_normals(v, f, normalise=True):
    """Area-weighted per-vertex normals of one frame: (N, 3).  A vertex in no triangle (or whose sum vanishes) gets NaN."""
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n = np.zeros_like(v, dtype=np.float64)
    for c in range(3):
        np.add.at(n, f[:, c], fn)
    if not normalise:
        return n
    with np.errstate(divide='ignore', invalid='ignore'):
        return n / np.linalg.norm(n, axis=1)[:, None]


def angle_between_row_vectors(a, b):
    """:73-90: degrees between corresponding rows, the cosine clipped to [-1, 1]."""
    with np.errstate(divide='ignore', invalid='ignore'):
        cos = np.einsum('ij,ij->i', a, b) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    return np.degrees(np.arccos(np.clip(cos, -1.0, 1.0)))


def denominator(frame_start, frame_end, n_verts):
    """:70 -- frame_end - frame_start, not the number of frames visited."""
    return np.sqrt(3 * (frame_end - frame_start) * n_verts)


def compute_accuracy(full, reduced, tris, frame_start, frame_end, frame_jump, normals=True):
    """The loop of :109-125 over range(frame_start, frame_end, frame_jump) on the (F, N, 3) arrays ``full`` and ``reduced``:
    frame_err, angle (F_sel, N), mesh_err (F_sel,), accum_norm, accum_angle (N,)."""
    N = full.shape[1]
    denom = denominator(frame_start, frame_end, N)
    accum_norm, accum_angle = np.zeros(N), np.zeros(N)
    frames_err, angles, mesh_err = [], [], []
    with np.errstate(divide='ignore', invalid='ignore'):
        for k in range(frame_start, frame_end, frame_jump):
            v, v_r = full[k], reduced[k]
            frame_err = ((v - v_r) ** 2).sum(axis=1) / (v ** 2).sum(axis=1) / denom            # :116
            mesh_err.append(np.linalg.norm(v - v_r) / np.linalg.norm(v) / denom)             # :117
            frames_err.append(frame_err)
            accum_norm += frame_err                                                          # :120
            if normals:
                ang = angle_between_row_vectors(per_vertex_normals(v, tris), per_vertex_normals(v_r, tris))     # :122-124
                angles.append(ang)
                accum_angle += ang                                                           # :125
    out = dict(frame_err=np.array(frames_err), mesh_err=np.array(mesh_err), accum_norm=accum_norm)
    if normals:
        out.update(angle=np.array(angles), accum_angle=accum_angle)
    return out


def stats_row(acc):
    """The 14 numbers behind ``r`` in a row of the commented-out writer (:132-137)."""
    fe, an = acc["frame_err"], acc["accum_norm"]
    row = [fe.min(), fe.mean(), fe.max(), fe.sum()]
    if "angle" in acc:
        ang, aa = acc["angle"], acc["accum_angle"]
        row += [ang.min(), ang.mean(), ang.max(), ang.sum()]
    else:
        row += [np.nan] * 4
    row += [an.min(), an.mean(), an.max()]
    row += [aa.min(), aa.mean(), aa.max()] if "angle" in acc else [np.nan] * 3
    return np.array(row)


def star_csr_brute(tris, n_verts):
    """Vertex stars by the definition: for each vertex, the triangles that have it as a corner, in increasing triangle number,
    once per corner."""
    ptr, star = [0], []
    for v in range(n_verts):
        for t, tri in enumerate(tris):
            star += [t] * int(sum(int(c) == v for c in tri))
        ptr.append(len(star))
    return np.array(ptr, dtype=np.int64), np.array(star, dtype=np.int64)


# ---- meshes
def grid_mesh(nx, ny, h=0.05, z=2.0):
    """nx x ny vertices in the plane z, spacing h, two triangles per cell, all counter-clockwise seen from +z."""
    x, y = np.meshgrid(np.arange(nx) * h, np.arange(ny) * h, indexing="ij")
    verts = np.stack([x.ravel(), y.ravel(), np.full(nx * ny, float(z))], axis=1)
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="ij")
    a = (i * ny + j).ravel()
    b, c, d = a + ny, a + ny + 1, a + 1
    return verts, np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)]).astype(np.int64)


def icosphere(subdiv):
    """Unit sphere from an icosahedron (12 vertices), each triangle split in four ``subdiv`` times; outward orientation."""
    p = (1 + 5 ** 0.5) / 2
    V = np.array([(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
                  (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)], dtype=np.float64)
    V /= np.linalg.norm(V, axis=1)[:, None]
    T = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    V = [tuple(v) for v in V]
    for _ in range(subdiv):
        mid, T2 = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                q = np.add(V[a], V[b])
                V.append(tuple(q / np.linalg.norm(q)))
                mid[key] = len(V) - 1
            return mid[key]
        for a, b, c in T:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            T2 += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        T = T2
    return np.array(V, dtype=np.float64), np.array(T, dtype=np.int64)


def animate(rest, n_frames, n_modes, seed, edge, amp=0.08, noise=0.03, coef_seed=0):
    """``rest`` displaced by ``n_modes`` smooth random modes (plane waves of wavelength >= 1 with random directions, total
    amplitude ~``amp``) plus white noise of ``noise`` x ``edge``: full numerical rank, no triangle folds over.  ``coef_seed``
    draws other coefficients and noise for the same modes (a held-out animation)."""
    rng = np.random.default_rng(seed)
    k = rng.normal(size=(n_modes, 3))
    k *= (2 * np.pi / rng.uniform(1.0, 3.0, size=n_modes) / np.linalg.norm(k, axis=1))[:, None]
    phase = rng.uniform(0, 2 * np.pi, size=n_modes)
    direc = rng.normal(size=(n_modes, 3))
    direc /= np.linalg.norm(direc, axis=1)[:, None]
    modes = np.sin(rest @ k.T + phase[None, :]).T[:, :, None] * direc[:, None, :]          # (m, N, 3)
    rng = np.random.default_rng([seed, coef_seed])
    coef = rng.normal(size=(n_frames, n_modes)) * (amp / np.sqrt(n_modes))
    out = rest[None] + np.tensordot(coef, modes, axes=1)
    out += rng.normal(size=out.shape) * (noise * edge)
    return out
