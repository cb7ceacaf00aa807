"""Small meshes for the device geodesics (csrc/asb_geodesic.hip): the smallest vertex counts at which each padding, tiling and
threshold edge of the kernels exists.  Plain NumPy / SciPy, no GPU import; tests/test_geodesic_model_cpu.py asserts the
properties listed here, tests/test_gpu_geodesic_small.py runs the device on them.

    case     n      why
    tiny     20     np = 32, nb = 1, nblk = 5; an OPEN patch (boundary vertices); one slab of two 16-blocks
    n127     127    np = 128: a single 128-tile, one padding row
    n128     128    np = n: no padding at all
    n129     129    np = 144: a ragged second tile 16 wide
    n255     255    np = 256, nb = 2
    n257     257    np = 272, nb = 3: the four ordered chunks of k_symv_finish hold 0, 1, 0, 2 partials
    n511     511    below the n >= 512 switch of geodesic.py: PCG for both steps, no coarse level
    n512     512    at the switch: Jacobi heat sweeps + two-level PCG
    n600     600    np = 608, nb = 5; the coarse level's nc is no multiple of 16 (ncp != nc)
    stride   4160   (n + 3) / 4 > 1024: the grid-stride loops of the batch kernels take a second turn; 3 slabs at the default target

(np = roundup(n, 16): the padded order of the dense inverses; nb = ceil(np / 128): tiles per side of k_symv_tiles;
 nblk = min((n + 3) / 4, 1024): blocks of the batch kernels.)
"""
import numpy as np

from oracle import asb_oracle as orc

SWEEP_LIMIT = 6000          # a quarter of heat_jacobi64's 24 000 sweeps


def torus(nu, nv, R=0.4, r=0.15):
    """A quasi-uniform triangle mesh with nu * nv vertices (a regular grid bent into a torus)."""
    th, ph = 2 * np.pi * np.arange(nu) / nu, 2 * np.pi * np.arange(nv) / nv
    T, P = np.meshgrid(th, ph, indexing="ij")
    V = np.stack([(R + r * np.cos(P)) * np.cos(T), (R + r * np.cos(P)) * np.sin(T), r * np.sin(P)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a, b = (i * nv + j).ravel(), (((i + 1) % nu) * nv + j).ravel()
    c, d = (i * nv + (j + 1) % nv).ravel(), (((i + 1) % nu) * nv + (j + 1) % nv).ravel()
    return V, np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)]).astype(np.int64)


def grid_patch(nx, ny, seed=0, jitter=0.15, bulge=0.2):
    """An open patch of nx * ny vertices: a unit-spaced grid, jittered in the plane and bulged out of it, two triangles
    per cell.  Boundary vertices have two to four neighbours."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing="ij")
    x = x + jitter * rng.uniform(-1, 1, size=x.shape)
    y = y + jitter * rng.uniform(-1, 1, size=y.shape)
    z = bulge * np.sin(np.pi * x / max(nx - 1, 1)) * np.sin(np.pi * y / max(ny - 1, 1)) * min(nx, ny)
    V = 0.1 * np.stack([x, y, z], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="ij")
    a, b, c, d = (i * ny + j).ravel(), ((i + 1) * ny + j).ravel(), (i * ny + j + 1).ravel(), ((i + 1) * ny + j + 1).ravel()
    return V, np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)]).astype(np.int64)


def split_face(V, T, t):
    """1 -> 3 split of triangle t at its centroid: one more vertex (the last), two more triangles; the corners of t gain a
    neighbour each and the new vertex has valence 3."""
    a, b, c = T[t]
    p = len(V)
    V2 = np.vstack([V, (V[a] + V[b] + V[c])[None] / 3.0])
    T2 = np.vstack([T[:t], T[t + 1:], [[a, b, p], [b, c, p], [c, a, p]]]).astype(np.int64)
    return V2, T2


def _split(mesh, faces):
    V, T = mesh
    for t in faces:
        V, T = split_face(V, T, t)
    return V, T


# name -> (builder, n, np, nb)
_BUILD = {
    "tiny": (lambda: grid_patch(4, 5, seed=3), 20, 32, 1),
    "n127": (lambda: orc.synth_mesh(5, 25, seed=2), 127, 128, 1),
    "n128": (lambda: _split(orc.synth_mesh(5, 25, seed=2), [40]), 128, 128, 1),
    "n129": (lambda: _split(orc.synth_mesh(5, 25, seed=2), [40, 130]), 129, 144, 2),
    "n255": (lambda: orc.synth_mesh(11, 23, seed=4), 255, 256, 2),
    "n257": (lambda: _split(grid_patch(15, 17, seed=5), [7, 300]), 257, 272, 3),
    "n511": (lambda: _split(torus(34, 15), [200]), 511, 512, 4),
    "n512": (lambda: torus(32, 16), 512, 512, 4),
    "n600": (lambda: torus(30, 20), 600, 608, 5),
    "stride": (lambda: torus(64, 65), 4160, 4160, 33),
}
CASES = tuple(_BUILD)
DENSE_CASES = ("tiny", "n127", "n128", "n129", "n255", "n257", "n600")
SLAB_CASES = (("tiny", 1536), ("n129", 1), ("n129", 40), ("n129", 100), ("n257", 1), ("n257", 40), ("n257", 100), ("stride", 1536))
# slabs bfs_slabs makes of each (tests/test_geodesic_model_cpu.py establishes them; the GPU module asserts n_slabs against them)
SLAB_COUNTS = {("tiny", 1536): 1, ("n129", 1): 7, ("n129", 40): 3, ("n129", 100): 2, ("n257", 1): 31, ("n257", 40): 6,
               ("n257", 100): 3, ("stride", 1536): 3}
SPARSE_CG_CASES = ("n127", "n511")                      # n < 512: PCG for the heat step too, no coarse level
SPARSE_SWEEP_CASES = ("n512", "n600", "stride")         # Jacobi heat sweeps + two-level PCG
_MESH = {}
_OPS = {}


def expected(name):
    """(n, np, nb) of the table"""
    return _BUILD[name][1:]


def mesh(name):
    """(V (n, 3) float64, T (m, 3) int64) of a named case; built once"""
    if name not in _MESH:
        V, T = _BUILD[name][0]()
        _MESH[name] = (np.ascontiguousarray(V, dtype=np.float64), np.ascontiguousarray(T, dtype=np.int64))
    return _MESH[name]


def operators(name):
    """(A_heat, L, G, D): the float64 operators GeodesicDistanceComputation.prepare() assembles for the case (what a device
    set-up uploads); built once"""
    if name not in _OPS:
        from animsnapbases_amd.geodesic import GeodesicDistanceComputation
        geo = GeodesicDistanceComputation(*mesh(name)).prepare()
        _OPS[name] = (geo._A_heat.tocsr(), geo._L.tocsr(), geo.G.tocsr(), geo.D.tocsr())
    return _OPS[name]


def padded(n):
    """(np, nb, nblk) as asb_geodesic.hip computes them"""
    np_ = (n + 15) // 16 * 16
    return np_, (np_ + 127) // 128, min((n + 3) // 4, 1024)


def jacobi_omega(A_heat):
    """the damping geodesic.py gives the heat step's Jacobi sweeps"""
    dg = A_heat.diagonal()
    g = float(((np.asarray(abs(A_heat).sum(axis=1)).ravel() - dg) / dg).max())
    return 1.0 if g <= 0.98 else min(1.0, 1.8 / (1.0 + g))


def jacobi_sweeps(A_heat):
    """(omega, rho, predicted sweeps): rho = spectral radius of I - omega D^-1 A (through the symmetric D^-1/2 A D^-1/2), the
    sweeps after which the relative change has fallen to heat_jacobi64's 2e-15"""
    omega = jacobi_omega(A_heat)
    A = np.asarray(A_heat.todense())
    s = 1.0 / np.sqrt(np.diag(A))
    mu = np.linalg.eigvalsh(A * s[:, None] * s[None, :])
    rho = float(np.abs(1.0 - omega * mu).max())
    return omega, rho, (np.log(2e-15) / np.log(rho) if 0 < rho < 1 else (0.0 if rho == 0 else np.inf))


def sources(n, count=64):
    """`count` source ids in shuffled order that include vertex 0 and vertex n - 1 and hold one duplicate pair (the last entry
    repeats the first); the others are the head of ONE fixed permutation of the interior ids, so the batches of every size
    draw from the same `count`-independent pool (count = 1: vertex n - 1 alone)."""
    if count == 1:
        return np.array([n - 1], dtype=np.int64)
    assert count >= 4
    pool = 1 + np.random.default_rng(1000 + n).permutation(n - 2)
    mid = pool[np.arange(count - 3) % pool.shape[0]]
    s = np.concatenate([[0, n - 1], mid])
    s = s[np.random.default_rng(count).permutation(s.shape[0])]
    return np.concatenate([s, s[:1]]).astype(np.int64)
