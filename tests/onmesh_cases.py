"""TEST HELPER: the inputs of tests/test_gpu_onmesh.py (meshes displaced by smooth random modes plus noise, tests/onmesh_model.py),
kept here so that tests/test_onmesh_cpu.py can check on the CPU what the tolerances of the GPU tests assume: the smallest
full-mesh vertex normal is far above rounding and no |x|^2 is below 1e-6."""
import numpy as np

import onmesh_model as om

# name -> (mesh, F, K, standarize, massWeight, rest shape, (frame_start, frame_end, frame_jump), r values, normals per r)
# The data have K + 8 modes and white noise, so r <= K stays below their rank.  F = 1 without standardising is a rank-1 tensor
# that r = 1 reproduces to rounding (both normals then agree to rounding, where arccos is ill-conditioned): its angle is
# checked for r = 0 only, where the reduced mesh is the single point 0 and every angle is NaN.
CASES = {
    "ico12_F1": (("ico", 0), 1, 1, False, False, "first", (0, 1, 1), (0, 1), (True, False)),
    "grid1000_F17": (("grid", 25, 40), 17, 8, True, True, "first", (2, 17, 3), (0, 1, 4, 8), (True,) * 4),
    "sphere642_F256": (("ico", 3), 256, 32, True, False, "average", (0, 256, 1), (0, 1, 16, 32), (True,) * 4),
    "grid3000_F257": (("grid", 50, 60), 257, 64, False, True, "first", (5, 200, 3), (0, 1, 32, 64), (True,) * 4),
    "grid20022_F2049": (("grid", 141, 142), 2049, 16, True, False, "average", (1500, 2049, 3), (8,), (True,)),
}


def mesh_of(spec):
    if spec[0] == "ico":
        rest, tris = om.icosphere(spec[1])
    else:
        rest, tris = om.grid_mesh(spec[1], spec[2])
    edge = np.linalg.norm(rest[tris[:, 0]] - rest[tris[:, 1]], axis=1).min()
    return rest, tris, edge


def make_case(name, n_frames=None, seed_shift=0):
    """(verts (F, N, 3), tris, mass or None) of a case; ``n_frames`` / ``seed_shift``: another animation of the same mesh and
    modes' family (a held-out one)."""
    spec, F, K, std, mw, rest_shape, rng_, rs, nm = CASES[name]
    rest, tris, edge = mesh_of(spec)
    seed = sum(map(ord, name))
    verts = om.animate(rest, F if n_frames is None else n_frames, K + 8, seed, edge, coef_seed=seed_shift)
    mass = np.random.default_rng(seed + 1).uniform(0.5, 2.0, size=rest.shape[0]) if mw else None
    return verts, tris, mass
