"""``posSnapshots`` -- drop-in mirror of the reference class (snapbases/posSnapshots.py)
whose tensor work runs on the MI355X through ``libasb_hip.so``.

Same constructor, attributes and method names as the reference (:33-61); the prepared
snapshot tensor lives in HBM in the vertex-major layout and is only copied
back when ``snapTensor`` is read.  With ``torch.distributed`` initialised the vertices are
sharded over the ranks (one GPU each): standardisation then needs two scalar all-reduces.
"""
import os
import sys

import numpy as np

from . import utils as _u
from .distributed import Comm
from .dynamics import ResidentDynamics
from .engine import HipEngine
from .geodesic import GeodesicDistanceComputation
from .utils import log_time


DENSE_GEODESIC_MAX_VERTS = 46000


class posSnapshots(ResidentDynamics):
    """Position snapshots: reads aligned ``(F, N, 3)`` frames, optionally mass-weights and
    standardises them (posSnapshots.py:26-31).  What the reference's class does not have is ``dynamics.ResidentDynamics``."""

    def __init__(self, input_train_animation_file, input_test_animation_file, rest_shape, masses_file,
                 tet_mesh_file, standarize=True, massWeight=True, *, verts=None, tris=None, test_verts=None,
                 test_tris=None, engine=None, comm=None, device_data=None):
        self.input_animation_file = input_train_animation_file
        self.input_test_animation_file = input_test_animation_file
        self.rest_shape = rest_shape            # "first" | "average"

        self.verts = verts
        self.test_verts = test_verts
        self.tris = tris
        self.test_tris = test_tris
        self.frs = 0
        self.nVerts = 0

        self.mean = None
        self.pre_scale_factor = 1
        self.massesFile = masses_file

        self.mass = None
        self.massL = None
        self.invMassL = None

        self._snapTensor = None
        self.compute_geodesic_distance = None
        self.tet_mesh = tet_mesh_file
        self.bending_indices = None             # constraint_projections("verts_bending"): the constrained vertices
        self.assembly_ST = None                 # constraint_forces / constraint_projections(wi=...): kind -> S^T (CSR)
        self.global_matrix = None               # global_solve_setup: A = M / dt^2 + sum w S^T S (CSR, N x N)
        self.global_solve_residual = None       # ... and max |A (A^-1 1) - 1| of the device's inverse

        # ---- device side ----
        self._comm = comm if comm is not None else Comm()
        self._engine = engine
        self._device_data = device_data         # (dev_ptr, F, N): synthetic data already in HBM (bench)
        self._in_memory = verts is not None or device_data is not None
        self.do_snapshots_precomputations(standarize, massWeight)

    # ------------------------------------------------------------------ construction helpers
    @classmethod
    def from_arrays(cls, verts, tris, rest_shape="first", masses_file="", standarize=True, massWeight=False,
                    engine=None, comm=None, mass=None, test_verts=None):
        """In-memory construction (no animation files): ``verts`` (F,N,3), ``tris`` (M,3) or None; ``test_verts``: the
        held-out (F',N,3) animation (posSnapshots.py:119-121), or None."""
        self = cls.__new__(cls)
        self._preset_mass = mass
        cls.__init__(self, None, None, rest_shape, masses_file, None, standarize, massWeight,
                     verts=np.asarray(verts), tris=tris, engine=engine, comm=comm,
                     test_verts=None if test_verts is None else np.asarray(test_verts))
        return self

    @classmethod
    def from_device(cls, dev_ptr, F, N, rest_shape="first", standarize=True, engine=None, comm=None, keepalive=None):
        """Adopts an ``(F, N, 3)`` float64 tensor that already sits in this rank's HBM (e.g. a
        torch tensor's ``data_ptr()``): this rank's shard of a larger problem, or all of it.  The tensor is
        standardised IN PLACE.  Without an ``engine`` the work is queued on torch's current stream when torch is loaded
        (so it is ordered after whatever produced the tensor); with an engine on another stream the caller must have
        synchronised the producer."""
        self = cls.__new__(cls)
        self._keepalive = keepalive
        if engine is None and "torch" in sys.modules:
            import torch
            if torch.cuda.is_available():
                engine = HipEngine(torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
        cls.__init__(self, None, None, rest_shape, "", None, standarize, False, engine=engine, comm=comm,
                     device_data=(int(dev_ptr), int(F), int(N)))
        return self

    # ------------------------------------------------------------------ properties
    @property
    def snapTensor(self):
        """The prepared tensor in the reference layout (F, N, 3); downloaded on first use."""
        if self._snapTensor is None and self._engine is not None and self._engine.n_loc:
            loc = self._engine.download_snapshots()
            self._snapTensor = self._comm.all_gather_rows(loc, self.nVerts, axis=1)
        return self._snapTensor

    @snapTensor.setter
    def snapTensor(self, value):
        self._snapTensor = value

    # ------------------------------------------------------------------ reference methods
    @log_time("")
    def do_snapshots_precomputations(self, standarize, massWeight):
        """posSnapshots.py:64-105."""
        self._standarize = bool(standarize)     # (the held-out animation of posComponents.reconstruction_errors repeats it)
        self.read()
        if self._engine is None:
            dev, stream = 0, None
            if self._comm.multi:
                import torch
                dev = torch.cuda.current_device()
                stream = torch.cuda.current_stream().cuda_stream
            self._engine = HipEngine(dev, stream)
        eng, comm = self._engine, self._comm

        massL = None
        fused = None
        if massWeight:
            self.read_factorize_masses()
            assert self.nVerts == self.massL.shape[0]
            massL = self.massL

        if self.rest_shape not in ("first", "average"):
            print('Error! unknown rest shape: ', self.rest_shape)
            sys.exit(1)

        if self._device_data is not None:
            ptr_, F, N = self._device_data
            # the adopted tensor IS this rank's shard; global N is the sum over ranks
            counts = comm.allreduce_sum(np.eye(comm.world)[comm.rank] * N) if comm.multi else np.array([N])
            self._shards = []
            v0 = 0
            for n in counts.astype(np.int64):
                self._shards.append((v0, int(n)))
                v0 += int(n)
            self.nVerts = int(counts.sum())
            self.frs = F
            code = 0 if self.rest_shape == "first" else 1
            if hasattr(eng, "adopt_device_rest"):       # layout change + rest shape (+ sums for the std) in one sweep
                fused = eng.adopt_device_rest(ptr_, F, N, None, self._shards[comm.rank][0], self.nVerts, code, standarize)
            else:
                eng.adopt_device(ptr_, F, N, None, self._shards[comm.rank][0], self.nVerts)
        else:
            v0, n_loc = comm.my_shard(self.nVerts)
            self._shards = comm.shards(self.nVerts)
            if min(n for _, n in self._shards) == 0:        # every rank sees the same partition and raises together
                raise ValueError("%d vertices cannot be sharded over %d ranks: every rank needs at least one vertex"
                                 % (self.nVerts, comm.world))
            code = 0 if self.rest_shape == "first" else 1
            if hasattr(eng, "upload_rest"):             # (:73, :82, :85-89) copy + M^{1/2} X, vertex-major, rest shape: one sweep
                fused = eng.upload_rest(self.verts, v0, n_loc, massL, code, standarize)
            else:
                eng.upload(self.verts, v0, n_loc, massL)

        # rest shape (:85-89); the mean row is subtracted only when standardising (:168)
        code = 0 if self.rest_shape == "first" else 1
        local_sum, local_sumsq = fused if fused is not None else (eng.center(code, standarize), None)
        self.mean = comm.all_gather_rows(eng.get_mean(), self.nVerts, axis=0)

        # geodesics on the NON-weighted shape (:96-99); host SciPy
        if self.tris is not None and self.verts is not None:
            shape0 = self.verts[0] if self.rest_shape == "first" else np.mean(self.verts, axis=0)
            # "dense" (default up to DENSE_GEODESIC_MAX_VERTS): both SPD systems inverted once on the device, a query =
            # gather + one dense product; the N x N inverses cost N^3 flop each and 8 N^2 bytes, so larger meshes take
            # "slab" (round 4): a DIRECT block-tridiagonal factorisation over breadth-first slabs of the mesh graph, robust
            # on graded meshes.  Opt-in: "device" (round 2's sparse batched PCG with a two-level preconditioner + Jacobi-sweep
            # heat step; refuses badly graded meshes), ASB_GEODESIC=host (SciPy SuperLU, what the reference does).
            mode = os.environ.get("ASB_GEODESIC", getattr(self, "geodesic_backend", "auto"))
            if mode == "auto":
                if not hasattr(eng, "geodesic_setup"):          # CPU test double of the engine (tests only)
                    mode = "host"
                elif self.nVerts <= DENSE_GEODESIC_MAX_VERTS:
                    mode = "dense"
                else:                                           # two N x N inverses no longer fit / pay: the slab factorisation
                    mode = "slab"
            self.compute_geodesic_distance = GeodesicDistanceComputation(
                shape0, self.tris, engine=eng if mode in ("dense", "device", "slab") else None,
                backend={"dense": "dense", "slab": "slab"}.get(mode, "pcg"))

        if standarize:
            self.standarize(_local_sum=local_sum, _local_sumsq=local_sumsq)
        print('Snapshots ready... Volkwein (' + str(massWeight) + '), standarized (' + str(standarize) + ').')

    @log_time("")
    def read(self):
        """posSnapshots.py:108-121."""
        if self._device_data is not None:
            return
        if not self._in_memory:
            self.verts, self.tris = _u.read_animation(self.input_animation_file)
        self.verts = np.asarray(self.verts).astype(float)
        self.frs, self.nVerts, _ = self.verts.shape
        print("Vertices: ", self.nVerts)
        print("Faces: ", 0 if self.tris is None else self.tris.shape[0])
        print("Frames: ", self.frs)
        if not self._in_memory and self.input_test_animation_file:
            self.test_verts, self.test_tris = _u.read_animation(self.input_test_animation_file)

    @log_time("")
    def read_factorize_masses(self, mass_on_tet_mesh=False):
        """posSnapshots.py:124-160.  The reference factorises the dense N x N ``diag(mass)``
        (Cholesky + inverse, O(N^3)); for a diagonal matrix that is sqrt / reciprocal."""
        N = self.nVerts
        preset = getattr(self, "_preset_mass", None)
        if preset is not None:
            Mass_mat = np.asarray(preset, dtype=np.float64).copy()
        elif not self.massesFile or not os.path.exists(self.massesFile):
            if mass_on_tet_mesh:      # (:133-135: igl.massmatrix on the tetrahedral mesh -- barycentric lumping, restated)
                _, self.tets, _ = _u.read_mesh_file(self.tet_mesh)
                Mass_mat = _u.tet_barycentric_vertex_masses(self.verts[0], self.tets)
            else:
                Mass_mat = _u.voronoi_vertex_masses(self.verts[0], self.tris)
            Mass_mat = Mass_mat / Mass_mat.sum() * 2
        else:
            Mass_mat = np.zeros(N)
            try:
                Mass_mat = _u.read_mass_bin(self.massesFile, N)
            except IOError:
                print(self.massesFile + " could not be read")
        self.mass = Mass_mat.copy()
        self.massL = np.sqrt(Mass_mat)
        self.invMassL = 1.0 / self.massL

    @log_time("")
    def standarize(self, _local_sum=None, _local_sumsq=None):
        """posSnapshots.py:163-172: after the mean row is gone, divide by the population
        standard deviation of ALL entries (np.std).  When the layout-change sweep already delivered sum(x) and sum(x^2),
        var = sum(x^2)/n - mu^2 (relative error eps (1 + mu^2/var)); only if the mean dominates (mu^2 > 10 var) the exact
        second pass over the tensor is taken."""
        eng, comm = self._engine, self._comm
        if _local_sum is None:
            _local_sum = eng.center(0 if self.rest_shape == "first" else 1, True)
        count = float(self.frs) * float(self.nVerts) * 3.0
        var = None
        if _local_sumsq is not None:
            tot = comm.allreduce_sum([_local_sum, _local_sumsq])
            mu = tot[0] / count
            v = tot[1] / count - mu * mu
            if v > 0 and mu * mu <= 10.0 * v:
                var = v
        else:
            mu = comm.allreduce_sum(_local_sum)[0] / count
        if var is None:
            var = comm.allreduce_sum(eng.sqdev(mu))[0] / count
        self.pre_scale_factor = 1 / np.sqrt(var)
        eng.scale(self.pre_scale_factor)
        self._snapTensor = None
