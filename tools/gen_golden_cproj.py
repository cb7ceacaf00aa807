"""Writes tests/golden/cproj_<kind>.npz from the UNMODIFIED reference classes of
projective_dynamics/Constraint_projections.py (CPU only; never imported by a test).

    python tools/gen_golden_cproj.py

Each file: ``rest`` (N, 3), ``elements``, ``frames`` (F, N, 3), ``expected`` (F, e p, 3) stacked as Simulators.py:655-724
stacks ``get_pi`` (rows p i .. p i + p of element i), ``sigma`` = [sigma_min, sigma_max] and the reference's rest tables.
Frame 0 is the rest pose; the others rotate, stretch, shear and perturb it so that both clamps act, and for the tetrahedra
some frames reflect single elements.  Before writing, the script asserts that every (element, frame) keeps the reference away
from its own discontinuities (these are conditions on the fixture, not tolerances).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.ref_import import REF_ROOT, _stub, install_stubs      # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SIGMA = (0.9, 1.1)
N_FRAMES = 130


def import_reference_projections():
    install_stubs()
    _stub("igl.copyleft")
    _stub("igl.copyleft.tetgen")
    sys.path.insert(0, os.path.join(REF_ROOT, "projective_dynamics"))
    import Constraint_projections as CP
    assert os.path.realpath(CP.__file__).startswith(os.path.realpath(REF_ROOT))
    return CP


# ------------------------------------------------------------------ meshes
def box_tets(nx=3, ny=3, nz=2, h=0.5):
    """nx x ny x nz vertices, every cell split into the six tetrahedra along its main diagonal."""
    vid = lambda i, j, k: (i * ny + j) * nz + k
    V = np.array([[i * h, j * h, k * h] for i in range(nx) for j in range(ny) for k in range(nz)], dtype=np.float64)
    T = []
    perms = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
    for i in range(nx - 1):
        for j in range(ny - 1):
            for k in range(nz - 1):
                for pm in perms:
                    c = [i, j, k]
                    tet = [vid(*c)]
                    for a in pm:
                        c[a] += 1
                        tet.append(vid(*c))
                    T.append(tet)
    return V, np.array(T, dtype=np.int64)


def edges_of(simplices):
    S = np.asarray(simplices)
    k = S.shape[1]
    e = np.concatenate([S[:, [a, b]] for a in range(k) for b in range(a + 1, k)])
    return np.unique(np.sort(e, axis=1), axis=0)


def tri_grid(nx=6, ny=5, h=0.25):
    """nx x ny cells (two triangles each) on a gently curved sheet; the boundary stays open."""
    vid = lambda i, j: i * (ny + 1) + j
    V = np.array([[i * h, j * h, 0.0] for i in range(nx + 1) for j in range(ny + 1)], dtype=np.float64)
    V[:, 2] = 0.15 * np.sin(2.1 * V[:, 0] + 0.3) * np.cos(1.7 * V[:, 1]) + 0.1 * V[:, 0] * V[:, 1]
    T = []
    for i in range(nx):
        for j in range(ny):
            a, b, c, d = vid(i, j), vid(i + 1, j), vid(i + 1, j + 1), vid(i, j + 1)
            T += [[a, b, c], [a, c, d]] if (i + j) % 2 == 0 else [[a, b, d], [b, c, d]]
    return V, np.array(T, dtype=np.int64)


def octahedron_subdivided():
    V = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    T = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
    V = [np.array(v, dtype=np.float64) for v in V]
    mid, out = {}, []

    def m(a, b):
        key = (min(a, b), max(a, b))
        if key not in mid:
            p = V[a] + V[b]
            V.append(p / np.linalg.norm(p))
            mid[key] = len(V) - 1
        return mid[key]

    for a, b, c in T:
        ab, bc, ca = m(a, b), m(b, c), m(c, a)
        out += [[a, ab, ca], [ab, b, bc], [ca, bc, c], [ab, bc, ca]]
    V = np.array(V) * np.array([0.6, 0.5, 0.4])            # an ellipsoid: the rest curvature varies over the vertices
    return V, np.array(out, dtype=np.int64)


def dyadic(V, bits=24):
    """Coordinates on a 2^-bits grid: DeformableMesh's +2 height shift of the rest pose is then exact."""
    return np.round(V * 2.0 ** bits) / 2.0 ** bits


# ------------------------------------------------------------------ frames
def rot(axis, th):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def animate(rest, n_frames, rng, noise, amp=1.0, fold=0.0, axis=(1, 2, 3)):
    """fold: the z coordinates are scaled by cos(fold f) first, so a curved sheet flattens and bends the other way."""
    c = rest.mean(axis=0)
    out = np.empty((n_frames,) + rest.shape)
    for f in range(n_frames):
        g = min(1.0, f / 10.0)
        S = np.diag([1 + amp * 0.35 * g * np.sin(0.11 * f), 1 - amp * 0.3 * g * np.sin(0.07 * f + 1), 1 + amp * 0.25 * g * np.cos(0.05 * f)])
        S[0, 1] = amp * 0.2 * g * np.sin(0.09 * f)
        A = rot(axis, 0.05 * f) @ S
        rf = rest * np.array([1.0, 1.0, np.cos(fold * f)])
        out[f] = (rf - c) @ A.T + c + g * np.array([0.02 * f, 0.0, 0.01 * f]) + g * noise * rng.standard_normal(rest.shape)
    out[0] = rest
    return out


def tet_F(rest, tets, frames):
    p4 = rest[tets[:, 3]]
    Dm = np.stack([rest[tets[:, 0]] - p4, rest[tets[:, 1]] - p4, rest[tets[:, 2]] - p4], axis=2)
    x4 = frames[:, tets[:, 3]]
    Ds = np.stack([frames[:, tets[:, 0]] - x4, frames[:, tets[:, 1]] - x4, frames[:, tets[:, 2]] - x4], axis=3)
    return Ds @ np.linalg.inv(Dm)[None]


def tet_conditions(Fm):
    s = np.linalg.svd(Fm, compute_uv=False)
    return (s[..., 2] / s[..., 0] >= 1e-3) & (s[..., 1] + s[..., 2] >= 1e-2) & (np.abs(np.linalg.det(Fm)) >= 1e-3)


def reflect_some(rest, tets, frames):
    """Every ninth frame: one vertex of one tetrahedron is pushed through the opposite face (1.6 x its height), which inverts
    that element; the first candidate that keeps every element of the frame within the conditions is taken."""
    n_inv = 0
    for f in range(4, frames.shape[0], 9):
        for t in [(7 * f + s) % tets.shape[0] for s in range(tets.shape[0])]:
            x = frames[f].copy()
            a, b, c, d = tets[t]
            n = np.cross(x[c] - x[b], x[d] - x[b])
            n /= np.linalg.norm(n)
            x[a] = x[a] - 1.6 * np.dot(x[a] - x[b], n) * n
            Fm = tet_F(rest, tets, x[None])
            if tet_conditions(Fm).all() and (np.linalg.det(Fm) < 0).any():
                frames[f] = x
                n_inv += int((np.linalg.det(Fm) < 0).sum())
                break
    return n_inv


# ------------------------------------------------------------------ reference runs
def stack(constraints, frames, p):
    out = np.zeros((frames.shape[0], len(constraints) * p, 3))
    for f in range(frames.shape[0]):
        q = frames[f].reshape(-1)
        for i, c in enumerate(constraints):
            if p == 1:
                out[f, i, :] = c.get_pi(q)
            else:
                out[f, p * i:p * i + p, :] = c.get_pi(q)
    return out


def save(name, **arrays):
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez(path, **arrays)
    size = os.path.getsize(path)
    assert size < (1 << 20), (name, size)
    print("%-40s %7.1f KB" % (os.path.basename(path), size / 1024.0))


def main():
    CP = import_reference_projections()
    rng = np.random.default_rng(20240607)
    sig = np.array(SIGMA)

    # ---- tetrahedra (and the edges of the same box)
    rest, tets = box_tets()
    tets = np.concatenate([tets, tets[:, [1, 2, 0, 3]], tets[:, [0, 1, 3, 2]]])[:68]        # re-ordered copies: other Dm, one odd
    frames = animate(rest, N_FRAMES, rng, 0.01)
    n_inv = reflect_some(rest, tets, frames)
    Fm = tet_F(rest, tets, frames)
    assert tet_conditions(Fm).all()
    assert n_inv >= 10, n_inv
    s = np.linalg.svd(Fm, compute_uv=False)
    assert (s < SIGMA[0]).any() and (s > SIGMA[1]).any()
    print("tets: %d inverted (element, frame) pairs, sigma in [%.3g, %.3g]" % (n_inv, s.min(), s.max()))
    cs = [CP.TetStrainConstraint(t.tolist(), 1.0, rest, *SIGMA) for t in tets]
    save("cproj_tets_strain", rest=rest, elements=tets, frames=frames, expected=stack(cs, frames, 3), sigma=sig,
         DmInv=np.array([c.DmInv for c in cs]))
    cs = [CP.TetDeformationGradientConstraint(t.tolist(), 1.0, rest) for t in tets]
    save("cproj_tets_deformation_gradient", rest=rest, elements=tets, frames=frames, expected=stack(cs, frames, 3), sigma=sig,
         DmInv=np.array([c.DmInv for c in cs]))

    E = edges_of(tets)
    E = np.concatenate([E, E[:15, ::-1]])[:68]
    fr_e = animate(rest, N_FRAMES, rng, 0.01)
    assert (np.linalg.norm(fr_e[:, E[:, 0]] - fr_e[:, E[:, 1]], axis=2) > 0).all()
    cs = [CP.EdgeSpringConstraint(e.tolist(), 1.0, rest) for e in E]
    save("cproj_edge_spring", rest=rest, elements=E, frames=fr_e, expected=stack(cs, fr_e, 1), sigma=sig,
         d=np.array([c.d for c in cs]))
    # one deliberately collapsed edge, in its own file: get_pi returns None (:303-304), which a float row stores as NaN
    E5, fr_c = E[:5], fr_e[:4].copy()
    fr_c[2, E5[3, 1]] = fr_c[2, E5[3, 0]]
    cs = [CP.EdgeSpringConstraint(e.tolist(), 1.0, rest) for e in E5]
    exp = stack(cs, fr_c, 1)
    assert np.isnan(exp[2, 3]).all() and np.isnan(exp).sum() == 3
    save("cproj_edge_spring_collapsed", rest=rest, elements=E5, frames=fr_c, expected=exp, sigma=sig)

    # ---- triangles: the open grid
    rest_g, tris_g = tri_grid()
    rest_g = dyadic(rest_g)
    tris_e = np.concatenate([tris_g, tris_g[:12][:, [1, 2, 0]]])[:68]
    # (the projection works in the REST tangent plane of each triangle, :416-417: the sheet turns about its own normal only)
    fr_g = animate(rest_g, N_FRAMES, rng, 0.004, axis=(0.02, 0.01, 1))
    cs = [CP.TriStrainConstraint(t.tolist(), 1.0, rest_g, *SIGMA) for t in tris_e]
    P = np.array([c.P for c in cs])
    Ds = np.stack([fr_g[:, tris_e[:, 1]] - fr_g[:, tris_e[:, 0]], fr_g[:, tris_e[:, 2]] - fr_g[:, tris_e[:, 0]]], axis=3)
    s2 = np.linalg.svd(np.einsum("tij,ftik->ftjk", P, Ds) @ np.array([c.DmInv for c in cs])[None], compute_uv=False)
    assert (s2[..., 1] >= 1e-3).all() and (s2 < SIGMA[0]).any() and (s2 > SIGMA[1]).any()
    save("cproj_tris_strain", rest=rest_g, elements=tris_e, frames=fr_g, expected=stack(cs, fr_g, 2), sigma=sig, P=P,
         DmInv=np.array([c.DmInv for c in cs]))

    # ---- bending: the open grid (boundary vertices skipped) and the closed octahedron (every vertex constrained)
    for tag, (V, T), noise in (("grid", (rest_g, tris_g), 0.004), ("closed", octahedron_subdivided(), 0.01)):
        V = dyadic(V)
        fr = animate(V, 67, rng, noise, amp=0.6, fold=0.11)
        n_flip = 0
        mesh = CP.DeformableMesh(V.copy(), T)
        mesh.add_vertex_bending_constraint(1.0)
        cs = mesh.verts_bending_constraints
        assert np.array_equal(mesh.init_positions - np.array([0.0, 2.0, 0.0]), V)         # the height shift was exact
        for f in range(fr.shape[0]):                  # the two thresholds and the flip test stay far from their switches
            q = fr[f].reshape(-1)
            for c in cs:
                ss = np.zeros(3)
                for e, w in zip(c.vertex_star, c.cotan_weights):
                    ss += (q[3 * c.v_ind:3 * c.v_ind + 3] - q[3 * e.v2:3 * e.v2 + 3]) * w
                nrm = np.linalg.norm(ss)
                assert nrm >= 1e-3, (tag, f, c.v_ind, nrm)
                dot = c.tri_normal @ (ss * (c.rest_mean_curvature / nrm))
                assert abs(dot * c.dot_with_normal) >= 1e-6, (tag, f, c.v_ind, dot * c.dot_with_normal)
                n_flip += int(dot * c.dot_with_normal < 0)
        exp = stack(cs, fr, 1)
        if tag == "closed":
            assert len(cs) == V.shape[0]
        else:
            assert 0 < len(cs) < V.shape[0]
        print("bending %s: %d of %d vertices, %d flipped entries" % (tag, len(cs), V.shape[0], n_flip))
        assert n_flip > 0
        save("cproj_verts_bending_" + tag, rest=V, elements=T, frames=fr, expected=exp, sigma=sig,
             indices=np.array(mesh.verts_bending_indicies, dtype=np.int64),
             star_ptr=np.cumsum([0] + [len(c.vertex_star) for c in cs]).astype(np.int64),
             star_idx=np.array([e.v2 for c in cs for e in c.vertex_star], dtype=np.int64),
             weights=np.concatenate([c.cotan_weights for c in cs]),
             rest_curvature=np.array([c.rest_mean_curvature for c in cs]), normal=np.array([c.tri_normal for c in cs]),
             dot_with_normal=np.array([c.dot_with_normal for c in cs]))


if __name__ == "__main__":
    main()
