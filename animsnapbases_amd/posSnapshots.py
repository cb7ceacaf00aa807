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

from . import projections as _proj
from . import reduced as _red
from . import utils as _u
from .distributed import Comm
from .engine import HipEngine
from .geodesic import GeodesicDistanceComputation
from .utils import log_time


DENSE_GEODESIC_MAX_VERTS = 46000


class posSnapshots:
    """Position snapshots: reads aligned ``(F, N, 3)`` frames, optionally mass-weights and
    standardises them (posSnapshots.py:26-31)."""

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

    # ------------------------------------------------------------------ extras: constraint projections of the animation
    def _cproj_args(self, kind, elements, rest_positions, sigma_min, sigma_max, animation, frame_start, frame_end, frame_jump):
        """The checks shared by ``constraint_projections`` and ``constraint_forces``: the rest set-up of the kind, the held-out
        animation (None: the training tensor) and the end of the frame range."""
        if kind not in _proj.KINDS:
            raise ValueError("unknown projection kind %r: one of %s" % (kind, ", ".join(sorted(_proj.KINDS))))
        if self._comm.multi:
            raise NotImplementedError("constraint_projections on several ranks: elements straddle the vertex shards and no "
                                      "halo of positions is built")
        if not sigma_min <= sigma_max:
            raise ValueError("sigma_min %r > sigma_max %r" % (sigma_min, sigma_max))
        if isinstance(animation, str) and animation not in ("train", "test"):
            raise ValueError("animation must be 'train', 'test' or an (F', N, 3) array, not %r" % (animation,))
        if elements is None:
            if kind != "verts_bending" or self.tris is None:
                raise ValueError("%s: no elements given%s" % (kind, " and the snapshots have no triangles" if kind == "verts_bending" else ""))
            elements = self.tris
        train = isinstance(animation, str) and animation == "train"
        Y = None
        if train:
            F = self.frs
        else:
            Y = self.test_verts if isinstance(animation, str) else animation
            if Y is None:
                raise ValueError("no test animation (test_verts is None)")
            Y = np.asarray(Y, dtype=np.float64)
            if Y.ndim != 3 or Y.shape[1:] != (self.nVerts, 3) or Y.shape[0] < 1:
                raise ValueError("held-out animation of shape %s: (F', %d, 3) expected" % (Y.shape, self.nVerts))
            F = Y.shape[0]
        frame_end = F if frame_end is None else frame_end
        if frame_jump < 1 or frame_start < 0 or frame_end > F or frame_start >= frame_end:
            raise ValueError("empty frame range: range(%r, %r, %r) selects none of the %d frames"
                             % (frame_start, frame_end, frame_jump, F))
        if rest_positions is None:
            if self.verts is not None:
                rest_positions = self.verts[0]
            else:                                   # an adopted device tensor: frame 0 back in world space
                rest_positions = self.snapTensor[0] / self.pre_scale_factor + (self.mean if self._standarize else 0.0)
        rest = np.asarray(rest_positions, dtype=np.float64)
        if rest.shape != (self.nVerts, 3):
            raise ValueError("rest positions of shape %s: (%d, 3) expected" % (rest.shape, self.nVerts))
        return _proj.build_setup(kind, elements, rest), Y, frame_end

    def constraint_projections(self, kind, elements=None, rest_positions=None, sigma_min=1.0, sigma_max=1.0, animation="train",
                               frame_start=0, frame_end=None, frame_jump=1, wi=None):
        """Extra (not in the reference's class): the constraint-projection snapshots the reference's projective-dynamics
        simulator records (Simulators.py:655-724) -- ``get_pi`` of every element for every frame
        (projective_dynamics/Constraint_projections.py) -- computed on the device from the resident animation in world space
        (mass weighting, mean row and scale undone), for the frames range(frame_start, frame_end, frame_jump).

        ``kind``: "edge_spring" (elements (E, 2)), "tris_strain" ((T, 3)), "tets_strain" / "tets_deformation_gradient"
        ((T, 4)) or "verts_bending" (elements: the (M, 3) triangles, None = ``self.tris``; the constrained vertices are left
        in ``self.bending_indices``).  ``rest_positions`` (N, 3): default frame 0 of the world-space input.  ``sigma_min`` /
        ``sigma_max``: the clamp of the strain kinds.  ``animation``: "train", "test" (``test_verts``) or an (F', N, 3) array.
        ``wi``: the constraint weight; when given, the kind's weighted differential operator S^T (``projections.assembly_ST``)
        is left in ``self.assembly_ST[kind]``.

        Returns ``(tensor, F', rows)``: a ``torch.float64`` device tensor (F', rows, 3), rows = elements x p, allocated here
        through torch and owned by the caller (what ``nonlinearSnapshots(frames_device=...)`` adopts).  One rank only."""
        setup, Y, frame_end = self._cproj_args(kind, elements, rest_positions, sigma_min, sigma_max, animation, frame_start,
                                               frame_end, frame_jump)
        St = None if wi is None else _proj.assembly_ST(setup, self.nVerts, wi)
        import torch
        eng = self._engine
        if Y is not None:
            eng.heldout_upload(Y, self.massL, self._standarize, self.pre_scale_factor)
        eng.cproj_setup(setup)
        n_sel = len(range(frame_start, frame_end, frame_jump))
        out = torch.empty((n_sel, setup.rows, 3), dtype=torch.float64, device="cuda:%d" % eng.device_id)
        eng.cproj_run(0 if Y is None else 1, frame_start, frame_end, frame_jump, self.invMassL, self._standarize,
                      self.pre_scale_factor, sigma_min, sigma_max, out.data_ptr())
        self.bending_indices = setup.bending_indices
        if St is not None:
            self.assembly_ST = {kind: St}
        return out, n_sel, setup.rows

    def _cforce_plan(self, kinds, animation, frame_start, frame_end, frame_jump, chunk_frames=None):
        """The checks of ``constraint_forces``, in its order: per kind ``(kind, setup, S^T, sigma_min, sigma_max, wi)``, the
        held-out animation (None: the training tensor) and the end of the frame range."""
        if not isinstance(kinds, (list, tuple)) or len(kinds) == 0:
            raise ValueError("constraint_forces: kinds must be a non-empty list of dicts, not %r" % (kinds,))
        if chunk_frames is not None and (int(chunk_frames) != chunk_frames or chunk_frames < 1):
            raise ValueError("constraint_forces: chunk_frames %r: a positive number of frames or None" % (chunk_frames,))
        known = ("kind", "elements", "wi", "rest_positions", "sigma_min", "sigma_max")
        plan, Y, end = [], None, frame_end
        for spec in kinds:
            if not isinstance(spec, dict) or "kind" not in spec:
                raise ValueError("constraint_forces: every entry of kinds is a dict with a 'kind', not %r" % (spec,))
            extra = sorted(set(spec) - set(known))
            if extra:
                raise ValueError("constraint_forces: unknown key %r (one of %s)" % (extra[0], ", ".join(known)))
            kind, smin, smax = spec["kind"], spec.get("sigma_min", 1.0), spec.get("sigma_max", 1.0)
            setup, Y, end = self._cproj_args(kind, spec.get("elements"), spec.get("rest_positions"), smin, smax, animation,
                                             frame_start, frame_end, frame_jump)
            if any(kind == q[0] for q in plan):
                raise ValueError("constraint_forces: kind %r is listed twice" % (kind,))
            plan.append((kind, setup, _proj.assembly_ST(setup, self.nVerts, spec.get("wi", 1.0)), smin, smax, spec.get("wi", 1.0)))
        return plan, Y, end

    def constraint_forces(self, kinds, animation="train", frame_start=0, frame_end=None, frame_jump=1, chunk_frames=None):
        """Extra (not in the reference's class): the constraint term of the global step's right-hand side,
        b[f] = sum_k S_k^T p_k(q_f) (``get_sum_ST_p``, Simulators.py:643-724), for the frames
        range(frame_start, frame_end, frame_jump) of the resident animation -- on the device, the projections p never formed
        at full size and never downloaded.

        ``kinds``: a non-empty list of dicts ``{"kind", "elements", "wi": 1.0, "rest_positions": None, "sigma_min": 1.0,
        "sigma_max": 1.0}`` with the meanings of ``constraint_projections``; a kind may be listed once.  The terms are added
        in list order.  ``chunk_frames``: frames per pass of the device (rounded up to a multiple of 16; None: as many as a
        256 MB scratch holds), which bounds the scratch and changes no bit of the result.

        Returns ``(tensor, F')``: a ``torch.float64`` device tensor (F', N, 3) in world space, allocated here through torch
        and owned by the caller -- the layout ``posSnapshots.from_device`` adopts.  Leaves ``self.assembly_ST`` (kind -> CSR)
        and ``self.bending_indices``.  One rank only."""
        plan, Y, end = self._cforce_plan(kinds, animation, frame_start, frame_end, frame_jump, chunk_frames)
        return self._cforce_run(plan, Y, frame_start, end, frame_jump, chunk_frames)

    def _cforce_run(self, plan, Y, frame_start, end, frame_jump, chunk_frames):
        """``constraint_forces`` for a plan of ``_cforce_plan``."""
        import torch
        eng = self._engine
        if Y is not None:
            eng.heldout_upload(Y, self.massL, self._standarize, self.pre_scale_factor)
        n_sel = len(range(frame_start, end, frame_jump))
        out = torch.empty((n_sel, self.nVerts, 3), dtype=torch.float64, device="cuda:%d" % eng.device_id)
        for i, (kind, setup, St, smin, smax, _wi) in enumerate(plan):
            eng.cproj_setup(setup)
            eng.cforce_run(0 if Y is None else 1, frame_start, end, frame_jump, self.invMassL, self._standarize,
                           self.pre_scale_factor, smin, smax, St, i > 0, 0 if chunk_frames is None else int(chunk_frames),
                           out.data_ptr())
        self.assembly_ST = {q[0]: q[2] for q in plan}
        bend = [q[1].bending_indices for q in plan if q[0] == "verts_bending"]
        self.bending_indices = bend[0] if bend else None
        return out, n_sel

    def _rforce_plan(self, kind, basis, elements, wi, reduction, rest_positions, sigma_min, sigma_max, animation, frame_start,
                     frame_end, frame_jump):
        """The checks of ``_cproj_args``, the kind's S^T and a function r -> ``reduced.ReducedOperator`` of the basis."""
        setup, Y, end = self._cproj_args(kind, elements, rest_positions, sigma_min, sigma_max, animation, frame_start, frame_end,
                                         frame_jump)
        if reduction not in _red.REDUCTIONS:
            raise ValueError("unknown reduction %r: one of %s" % (reduction, ", ".join(sorted(_red.REDUCTIONS))))
        St = _proj.assembly_ST(setup, self.nVerts, wi)
        data = _red.load_basis(basis)

        def operator(r):
            return _red.reduced_operator(data["components"], data["interpol_alphas"], data["Pt"], data["interpol_alpha_ranges"],
                                         r, setup.p, reduction, n_elements=setup.n_elem, verts_bending=kind == "verts_bending")
        return setup, Y, end, St, operator

    def _rforce_term(self, setup, op, which, frame_start, end, frame_jump, sigma_min, sigma_max):
        """One reduced term with the operator of the engine: only the sampled elements are set up and projected."""
        import torch
        eng = self._engine
        eng.cproj_setup(_proj.subset_setup(setup, op.elements))
        eng.rforce_solver(op.H, op.local_rows)
        n_sel = len(range(frame_start, end, frame_jump))
        out = torch.empty((n_sel, self.nVerts, 3), dtype=torch.float64, device="cuda:%d" % eng.device_id)
        eng.rforce_run(which, frame_start, end, frame_jump, self.invMassL, self._standarize, self.pre_scale_factor, sigma_min,
                       sigma_max, False, out.data_ptr())
        return out, n_sel

    def reduced_constraint_forces(self, kind, basis, num_components, elements=None, wi=1.0, reduction="deim_pod",
                                  rest_positions=None, sigma_min=1.0, sigma_max=1.0, animation="train", frame_start=0,
                                  frame_end=None, frame_jump=1):
        """Extra (not in the reference's class): the constraint term the reference's REDUCED simulator puts on the global
        step's right-hand side, b~[f] = S^T V (P^T V)^+ P^T p(q_f) per coordinate (Simulators.py:157-255, :366-399;
        ``reduced.reduced_operator``), for the frames range(frame_start, frame_end, frame_jump) of the resident animation.
        ``get_pi`` is evaluated at the interpolation elements only; S^T V is formed once on the device, sparse times dense.

        ``kind``, ``elements``, ``rest_positions``, ``sigma_min`` / ``sigma_max``, ``animation``: as ``constraint_projections``
        (``elements``: ALL elements of the kind, the ones the basis was built on); ``wi``: the constraint weight of S^T.
        ``basis``: a ``constraintsComponents`` with components and interpolation points, the path of the ``.npz`` of its
        ``store_components_n_interpol_points``, or a dict with the keys components, interpol_alphas, Pt,
        interpol_alpha_ranges.  ``num_components``: m.  ``reduction``: the simulator's
        ``constraint_projection_reduction_type`` ("deim_pod", "deim_pod_vectorized": single rows; "deim_pca_blocks",
        "geom_pca_blocks_withSt": whole blocks of p rows).

        Returns ``(tensor, F')``: a ``torch.float64`` device tensor (F', N, 3) in world space, the layout of
        ``constraint_forces``.  Leaves ``self.assembly_ST[kind]`` and ``self.bending_indices``.  One rank only."""
        setup, Y, end, St, operator = self._rforce_plan(kind, basis, elements, wi, reduction, rest_positions, sigma_min, sigma_max,
                                                        animation, frame_start, frame_end, frame_jump)
        op = operator(num_components)
        eng = self._engine
        if Y is not None:
            eng.heldout_upload(Y, self.massL, self._standarize, self.pre_scale_factor)
        eng.rforce_operator(St, op.V)
        out, n_sel = self._rforce_term(setup, op, 0 if Y is None else 1, frame_start, end, frame_jump, sigma_min, sigma_max)
        self.assembly_ST = {kind: St}
        self.bending_indices = setup.bending_indices
        return out, n_sel

    def reduced_force_errors(self, kind, basis, r_values, elements=None, wi=1.0, reduction="deim_pod", rest_positions=None,
                             sigma_min=1.0, sigma_max=1.0, animation="train", frame_start=0, frame_end=None, frame_jump=1,
                             per_frame=False):
        """Extra (not in the reference): how wrong the forces of the reduced simulation are -- for every r of ``r_values`` the
        reference's ``frobenius_error``, ``max_pointwise_error`` and ``relative_error_per_component``
        (constraintsComponents.py:524-556) of ``(b, b~_r)``, b the full term of ``constraint_forces`` for this kind and b~_r
        ``reduced_constraint_forces`` with r components, as five lists ``fro, max, rel_x, rel_y, rel_z``; with ``per_frame``
        a sixth value, the (len(r_values), F') array of |b[f] - b~_r[f]| / |b[f]| (Frobenius norms of the frame).  Arguments as
        ``reduced_constraint_forces``.  The full term is computed once, S^T V once for the largest r (prefixes of its
        columns serve the others); both tensors stay on the device and are compared there (asb_force_diff)."""
        setup, Y, end, St, operator = self._rforce_plan(kind, basis, elements, wi, reduction, rest_positions, sigma_min, sigma_max,
                                                        animation, frame_start, frame_end, frame_jump)
        r_values = [int(r) for r in r_values]
        ops = [operator(r) for r in r_values]
        if not ops:
            return self._diff_metrics(None, [], 0, per_frame)
        eng = self._engine
        full, n_sel = self.constraint_forces([dict(kind=kind, elements=elements, wi=wi, rest_positions=rest_positions,
                                                   sigma_min=sigma_min, sigma_max=sigma_max)], animation=animation,
                                             frame_start=frame_start, frame_end=end, frame_jump=frame_jump)
        eng.rforce_operator(St, ops[int(np.argmax(r_values))].V)
        which = 0 if Y is None else 1
        out = self._diff_metrics(full, (self._rforce_term(setup, op, which, frame_start, end, frame_jump, sigma_min, sigma_max)[0]
                                        for op in ops), n_sel, per_frame)
        self.assembly_ST = {kind: St}
        self.bending_indices = setup.bending_indices
        return out

    def _diff_metrics(self, full, others, n_sel, per_frame):
        """The reference's three metrics (constraintsComponents.py:524-556) of ``(full, t)`` for every device tensor ``t`` of
        ``others`` (made one at a time), through ``asb_force_diff``: the lists ``fro, max, rel_x, rel_y, rel_z`` and, with
        ``per_frame``, the (len(others), F') array of |full[f] - t[f]| / |full[f]|."""
        fro, mx, rel, frames = [], [], [[], [], []], []
        for t in others:
            sums, m, norms, pf = self._engine.force_diff(full.data_ptr(), t.data_ptr(), n_sel, self.nVerts, per_frame)
            with np.errstate(divide='ignore', invalid='ignore'):
                fro.append(float(np.sqrt(sums.sum())))
                mx.append(float(m / norms[3]))
                for d in range(3):
                    rel[d].append(float(np.sqrt(sums[d]) / np.sqrt(norms[d])))
                if per_frame:
                    frames.append(np.sqrt(pf[:, 0]) / np.sqrt(pf[:, 1]))
        if per_frame:
            return fro, mx, rel[0], rel[1], rel[2], np.array(frames).reshape(len(fro), -1) if fro else np.zeros((0, 0))
        return fro, mx, rel[0], rel[1], rel[2]

    # ------------------------------------------------------------------ extras: the global step of projective dynamics
    def _gstep_one_rank(self, who):
        if self._comm.multi:
            raise NotImplementedError("%s on several ranks: the system matrix couples the vertex shards and no distributed "
                                      "solve is built" % who)

    def _gstep_masses(self, masses):
        if masses is None:
            masses = self.mass
            if masses is None:
                raise ValueError("no vertex masses: the snapshots were built without mass weighting, pass masses=")
        return np.asarray(masses, dtype=np.float64)

    def global_solve_setup(self, kinds, dt, masses=None):
        """Extra (not in the reference's class): prepares the global step of the reference's projective-dynamics solver,
        ``prepare_global_matrix`` (Simulators.py:117-145), for this mesh: A = M / dt^2 + sum_i w_i S_i^T S_i is assembled on
        the host from the rest tables (``projections.global_matrix``: one N x N matrix serves the three coordinates) and
        inverted once on the device, where A^-1 stays until the next set-up.

        ``kinds``: the list of dicts of ``constraint_forces`` (same checks).  ``dt``: the time step h.  ``masses`` (N,): None
        takes the vertex masses the snapshots were mass-weighted with.  Leaves ``self.global_matrix`` (CSR) and
        ``self.global_solve_residual`` = max |A (A^-1 1) - 1| as the device computed it.  Cost: the host assembly and symmetry
        check, and on the device a dense N x N inversion (N^3 flop, 8 N^2 bytes); a set-up whose matrix equals the one the
        device already holds keeps that inverse.  N <= 46 000, one rank only."""
        self._gstep_one_rank("global_solve_setup")
        plan, _, _ = self._cforce_plan(kinds, "train", 0, None, 1)
        self._gstep_setup(plan, dt, self._gstep_masses(masses))

    def _gstep_setup(self, plan, dt, masses):
        A = _proj.global_matrix([(q[1], q[5]) for q in plan], self.nVerts, masses, dt)
        self.global_matrix, self.global_solve_residual = None, None
        resid = self._engine.gstep_held(A)
        if resid is None:
            resid = self._engine.gstep_setup(A)
        self.global_matrix, self.global_solve_residual = A, resid

    def global_solve(self, rhs):
        """Extra: q = A^-1 rhs per coordinate for the matrix of the last ``global_solve_setup``.  ``rhs``: a caller-owned
        ``torch.float64`` device tensor (F', N, 3), contiguous; returns a new one of the same shape, owned by the caller.  The
        sum over the vertices is never split: a frame's result does not depend on the frames around it."""
        self._gstep_one_rank("global_solve")
        if getattr(self, "global_matrix", None) is None:
            raise ValueError("global_solve: no system matrix on the device, call global_solve_setup first")
        import torch
        if not isinstance(rhs, torch.Tensor) or rhs.dtype != torch.float64 or not rhs.is_cuda:
            raise ValueError("global_solve: rhs must be a torch.float64 device tensor")
        if rhs.device.index != self._engine.device_id:
            raise ValueError("global_solve: rhs lives on %s, the snapshots on device %d" % (rhs.device, self._engine.device_id))
        if rhs.dim() != 3 or rhs.shape[0] < 1 or tuple(rhs.shape[1:]) != (self.nVerts, 3) or not rhs.is_contiguous():
            raise ValueError("global_solve: rhs of shape %s: a contiguous (F', %d, 3) expected" % (tuple(rhs.shape), self.nVerts))
        out = torch.empty_like(rhs)
        torch.cuda.current_stream(rhs.device).synchronize()         # whatever produced rhs is done before the engine reads it
        self._engine.gstep_run(rhs.data_ptr(), rhs.shape[0], out.data_ptr())
        return out

    @staticmethod
    def _gstep_explicit(dt, velocity, gravity):
        if velocity not in ("difference", "zero"):
            raise ValueError("velocity must be 'difference' or 'zero', not %r" % (velocity,))
        g = np.asarray(gravity, dtype=np.float64)
        if g.shape != (3,) or not np.isfinite(g).all():
            raise ValueError("gravity %r: three finite numbers expected" % (gravity,))
        try:
            h = float(dt)
        except (TypeError, ValueError):
            h = float("nan")
        if not np.isfinite(h) or h <= 0.0:
            raise ValueError("the time step dt must be finite and positive, not %r" % (dt,))
        return 1 if velocity == "difference" else 0, h * h * g

    def _gstep_inertia(self, rhs, masses, dt, mode, acc, which, frame_start, end, frame_jump):
        """rhs += M / dt^2 s of the selected frames."""
        self._engine.gstep_inertia(which, frame_start, end, frame_jump, self.invMassL, self._standarize, self.pre_scale_factor,
                                   masses * (1.0 / (float(dt) * float(dt))), mode, acc, rhs.data_ptr())

    def global_step(self, kinds, dt, masses=None, velocity="difference", gravity=(0.0, 0.0, 0.0), animation="train",
                    frame_start=0, frame_end=None, frame_jump=1, chunk_frames=None):
        """Extra: one local/global iteration of the reference's solver started at every selected frame of the resident
        animation (Simulators.py:494-526 with ``num_iterations`` = 1 and q = x_f):
        Phi(x_f; s_f) = A^-1 (M / dt^2 s_f + sum_k S_k^T p_k(x_f)), on the device.

        ``kinds``, ``animation``, the frame range and ``chunk_frames``: as ``constraint_forces``; ``dt``, ``masses``: as
        ``global_solve_setup``, whose work is done here first -- the matrix is assembled on every call, the dense inversion
        is paid only when the matrix differs from the one the device holds.  ``velocity``: "zero" takes the explicit state
        s_f = x_f + dt^2 g, "difference"
        s_f = 2 x_f - x_{f-1} + dt^2 g with f - 1 the ANIMATION's previous frame whatever ``frame_jump`` is (at frame 0:
        x_0), the velocity the reference carries from step to step (:531).  ``gravity``: the acceleration g.

        Returns ``(tensor, F')``: a ``torch.float64`` device tensor (F', N, 3) in world space, owned by the caller.  Further
        iterations are ``solve_frames``: they keep s_f fixed while q moves, which re-adopting the result with ``from_device``
        and stepping again would not.  One rank only."""
        self._gstep_one_rank("global_step")
        mode, acc = self._gstep_explicit(dt, velocity, gravity)
        m = self._gstep_masses(masses)
        plan, Y, end = self._cforce_plan(kinds, animation, frame_start, frame_end, frame_jump, chunk_frames)
        self._gstep_setup(plan, dt, m)
        b, n_sel = self._cforce_run(plan, Y, frame_start, end, frame_jump, chunk_frames)
        self._gstep_inertia(b, m, dt, mode, acc, 0 if Y is None else 1, frame_start, end, frame_jump)
        return self.global_solve(b), n_sel

    def reduced_global_step_errors(self, kind, basis, r_values, dt, masses=None, velocity="difference", gravity=(0.0, 0.0, 0.0),
                                   elements=None, wi=1.0, reduction="deim_pod", rest_positions=None, sigma_min=1.0,
                                   sigma_max=1.0, animation="train", frame_start=0, frame_end=None, frame_jump=1,
                                   per_frame=False):
        """Extra: how far the reduced right-hand side moves the vertices -- ``reduced_force_errors`` one line further down the
        iteration.  Cost beside that method's: the work of ``global_solve_setup`` once, one solve plus one per r.
        For every r of ``r_values`` the three metrics of ``(q, q~_r)``: q = ``global_step`` of this kind and
        q~_r the same step with b~_r of ``reduced_constraint_forces`` in place of b (same inertia term, same A^-1).  Arguments
        as ``reduced_force_errors`` plus ``dt``, ``masses``, ``velocity``, ``gravity`` of ``global_step``; the same five lists
        ``fro, max, rel_x, rel_y, rel_z`` and, with ``per_frame``, the (len(r_values), F') array |q[f] - q~_r[f]| / |q[f]|.
        The full step is computed once; every tensor stays on the device."""
        self._gstep_one_rank("reduced_global_step_errors")
        mode, acc = self._gstep_explicit(dt, velocity, gravity)
        m = self._gstep_masses(masses)
        setup, Y, end, St, operator = self._rforce_plan(kind, basis, elements, wi, reduction, rest_positions, sigma_min, sigma_max,
                                                        animation, frame_start, frame_end, frame_jump)
        r_values = [int(r) for r in r_values]
        ops = [operator(r) for r in r_values]
        if not ops:
            return self._diff_metrics(None, [], 0, per_frame)
        eng, which = self._engine, 0 if Y is None else 1
        spec = dict(kind=kind, elements=elements, wi=wi, rest_positions=rest_positions, sigma_min=sigma_min, sigma_max=sigma_max)
        plan, Y, end = self._cforce_plan([spec], animation, frame_start, end, frame_jump)
        self._gstep_setup(plan, dt, m)
        b, n_sel = self._cforce_run(plan, Y, frame_start, end, frame_jump, None)
        self._gstep_inertia(b, m, dt, mode, acc, which, frame_start, end, frame_jump)
        full = self.global_solve(b)
        del b
        eng.rforce_operator(St, ops[int(np.argmax(r_values))].V)

        def steps():
            for op in ops:
                red, _ = self._rforce_term(setup, op, which, frame_start, end, frame_jump, sigma_min, sigma_max)
                self._gstep_inertia(red, m, dt, mode, acc, which, frame_start, end, frame_jump)
                yield self.global_solve(red)
        out = self._diff_metrics(full, steps(), n_sel, per_frame)
        self.assembly_ST = {kind: St}
        self.bending_indices = setup.bending_indices
        return out

    # ------------------------------------------------------------------ extras: the solver's iterations
    _SOLVE_SCOPE = """Out of scope, as for ``global_step``: collision handling (``resolve_collision`` and the self-collision passes),
        positional constraints, velocities carried from one solved frame into the next (every selected frame is an independent
        solve from the animation's own x_f, x_{f-1}), the hyper-reduced operator A^-1 S^T V (a reduced iteration still pays the
        N^2 product) and several ranks."""

    def _solve_args(self, who, dt, velocity, gravity, num_iterations, start, masses):
        """The checks of the solve's own arguments, before anything touches the device: (mode, acc, masses, K)."""
        self._gstep_one_rank(who)
        mode, acc = self._gstep_explicit(dt, velocity, gravity)
        try:
            K = int(num_iterations)
        except (TypeError, ValueError):
            K = 0
        if K != num_iterations or K < 1:
            raise ValueError("%s: num_iterations %r: a positive number of iterations" % (who, num_iterations))
        if isinstance(start, str):
            if start not in ("explicit", "frame"):
                raise ValueError("%s: start must be 'explicit', 'frame' or a torch.float64 device tensor, not %r" % (who, start))
        else:
            import torch
            if not isinstance(start, torch.Tensor) or start.dtype != torch.float64 or not start.is_cuda:
                raise ValueError("%s: start must be 'explicit', 'frame' or a torch.float64 device tensor" % who)
        return mode, acc, self._gstep_masses(masses), K

    def _solve_plan(self, who, kinds, animation, frame_start, frame_end, frame_jump, chunk_frames):
        """``_cforce_plan`` of the kinds with their reduction keys taken off, and for the one entry that carries a ``basis``
        its index in the plan and r -> ``reduced.ReducedOperator``."""
        keys = ("basis", "num_components", "reduction")
        if not isinstance(kinds, (list, tuple)):
            raise ValueError("%s: kinds must be a non-empty list of dicts, not %r" % (who, kinds))
        plain, red = [], None
        for i, spec in enumerate(kinds):
            if isinstance(spec, dict) and any(k in spec for k in keys):
                if "basis" not in spec or "num_components" not in spec:
                    raise ValueError("%s: a reduced kind carries both 'basis' and 'num_components'" % who)
                if red is not None:
                    raise ValueError("%s: a second reduced kind (%r after %r): the engine holds one reduced operator"
                                     % (who, spec.get("kind"), kinds[red[0]].get("kind")))
                red = (i, spec)
                spec = {k: v for k, v in spec.items() if k not in keys}
            plain.append(spec)
        plan, Y, end = self._cforce_plan(plain, animation, frame_start, frame_end, frame_jump, chunk_frames)
        if red is None:
            return plan, Y, end, None
        i, spec = red
        setup, _, _, St, operator = self._rforce_plan(spec["kind"], spec["basis"], spec.get("elements"), spec.get("wi", 1.0),
                                                      spec.get("reduction", "deim_pod"), spec.get("rest_positions"),
                                                      spec.get("sigma_min", 1.0), spec.get("sigma_max", 1.0), animation, frame_start,
                                                      end, frame_jump)
        return plan, Y, end, (i, setup, St, operator)

    def _solve_start(self, who, start, n_sel):
        """(start code of the engine, device pointer or None); a tensor is checked as ``global_solve`` checks its rhs."""
        if isinstance(start, str):
            return (0 if start == "explicit" else 1), None
        if start.device.index != self._engine.device_id:
            raise ValueError("%s: start lives on %s, the snapshots on device %d" % (who, start.device, self._engine.device_id))
        if start.dim() != 3 or tuple(start.shape) != (n_sel, self.nVerts, 3) or not start.is_contiguous():
            raise ValueError("%s: start of shape %s: a contiguous (%d, %d, 3) expected" % (who, tuple(start.shape), n_sel, self.nVerts))
        return 2, start.data_ptr()

    def _solve_run(self, who, plan, red, Y, frame_start, end, frame_jump, chunk_frames, K, start, m, dt, mode, acc, history):
        """The solve for a plan whose matrix is on the device; ``red``: None or (index in the plan, full set-up, operator of the
        r in use), the engine's ``rforce_operator`` holding at least its columns."""
        import torch
        eng = self._engine
        n_sel = len(range(frame_start, end, frame_jump))
        code, ptr = self._solve_start(who, start, n_sel)
        if code == 2:
            torch.cuda.current_stream(start.device).synchronize()   # whatever produced start is done before the engine reads it
        if Y is not None:
            eng.heldout_upload(Y, self.massL, self._standarize, self.pre_scale_factor)
        eng.pdsolve_begin(0 if Y is None else 1, frame_start, end, frame_jump, self.invMassL, self._standarize, self.pre_scale_factor,
                          m * (1.0 / (float(dt) * float(dt))), mode, acc, code, ptr)
        for i, (_kind, setup, St, smin, smax, _wi) in enumerate(plan):
            if red is not None and red[0] == i:
                eng.cproj_setup(_proj.subset_setup(red[1], red[2].elements))
                eng.rforce_solver(red[2].H, red[2].local_rows)
                eng.pdsolve_slot(smin, smax, None)
            else:
                eng.cproj_setup(setup)
                eng.pdsolve_slot(smin, smax, St)
        out = torch.empty((n_sel, self.nVerts, 3), dtype=torch.float64, device="cuda:%d" % eng.device_id)
        hist = eng.pdsolve_iterate(K, 0 if chunk_frames is None else int(chunk_frames), out.data_ptr(), history)
        self.assembly_ST = {q[0]: q[2] for q in plan}
        bend = [q[1].bending_indices for q in plan if q[0] == "verts_bending"]
        self.bending_indices = bend[0] if bend else None
        if history:
            with np.errstate(divide='ignore', invalid='ignore'):
                return out, n_sel, np.sqrt(hist[:, :, 0]) / np.sqrt(hist[:, :, 1])
        return out, n_sel

    def solve_frames(self, kinds, dt, num_iterations=10, masses=None, velocity="difference", gravity=(0.0, 0.0, 0.0), start="explicit",
                     animation="train", frame_start=0, frame_end=None, frame_jump=1, chunk_frames=None, history=False):
        """Extra: the local/global iterations of the reference's solver (Simulators.py:494-526) for every selected frame of
        the resident animation, on the device: q_0 given, q_{k+1} = A^-1 (M / dt^2 s_f + sum_i S_i^T p_i(q_k)) for
        ``num_iterations`` iterations, the explicit state s_f held fixed while q moves.  The iterate stays on the device
        between iterations in the layout the projection kernels read; the kinds' tables and S^T are uploaded once per solve.

        ``kinds``: the list of dicts of ``constraint_forces``; ONE entry may also carry ``basis``, ``num_components`` and
        ``reduction`` (default "deim_pod") with the meanings of ``reduced_constraint_forces``: that kind's term is then the
        reduced one, as the simulator's per-group ``*_reduced`` flags choose.  A is always the full matrix of all listed kinds.
        ``dt``, ``masses``, ``velocity``, ``gravity``, ``animation``, the frame range and ``chunk_frames``: as ``global_step``.
        ``start``: "explicit" (q_0 = s_f, the reference's), "frame" (q_0 = x_f; one iteration is then ``global_step`` bit for
        bit) or a contiguous ``torch.float64`` device tensor (F', N, 3) -- a solve continued from an earlier result equals the
        longer solve bit for bit.  ``history``: also the (num_iterations, F') array of |q_{k+1} - q_k| / |q_{k+1}| (Frobenius
        norms of the frame).

        Returns ``(tensor, F')`` (``(tensor, F', steps)`` with ``history``): a ``torch.float64`` device tensor (F', N, 3) in
        world space, owned by the caller.  Device memory held by the engine beside A^-1: three times the result plus the
        projections of one chunk.  %s"""
        who = "solve_frames"
        mode, acc, m, K = self._solve_args(who, dt, velocity, gravity, num_iterations, start, masses)
        plan, Y, end, red = self._solve_plan(who, kinds, animation, frame_start, frame_end, frame_jump, chunk_frames)
        self._solve_start(who, start, len(range(frame_start, end, frame_jump)))
        if red is not None:
            op = red[3](int(kinds[red[0]]["num_components"]))
        self._gstep_setup(plan, dt, m)
        if red is not None:
            self._engine.rforce_operator(red[2], op.V)
            red = (red[0], red[1], op)
        return self._solve_run(who, plan, red, Y, frame_start, end, frame_jump, chunk_frames, K, start, m, dt, mode, acc, history)

    solve_frames.__doc__ %= _SOLVE_SCOPE

    def reduced_solve_errors(self, kind, basis, r_values, dt, num_iterations=10, masses=None, velocity="difference",
                             gravity=(0.0, 0.0, 0.0), start="explicit", elements=None, wi=1.0, reduction="deim_pod", rest_positions=None,
                             sigma_min=1.0, sigma_max=1.0, animation="train", frame_start=0, frame_end=None, frame_jump=1,
                             per_frame=False):
        """Extra: how far the DEIM-reduced simulation is from the full one after the solver's iterations -- for every r of
        ``r_values`` the three metrics of ``(q, q~_r)``, q = ``solve_frames`` of this kind and q~_r the same solve with the kind
        reduced to r components (same A^-1, same inertia term, same start).  Arguments as ``reduced_global_step_errors`` plus
        ``num_iterations`` and ``start``; the same five lists ``fro, max, rel_x, rel_y, rel_z`` and, with ``per_frame``, the
        (len(r_values), F') array |q[f] - q~_r[f]| / |q[f]|.  The full solve runs once, one reduced solve per r (S^T V once, for
        the largest r); every tensor stays on the device and is compared there.  With ``num_iterations=1, start="frame"`` these
        are the numbers of ``reduced_global_step_errors``.  %s"""
        who = "reduced_solve_errors"
        mode, acc, m, K = self._solve_args(who, dt, velocity, gravity, num_iterations, start, masses)
        spec = dict(kind=kind, elements=elements, wi=wi, rest_positions=rest_positions, sigma_min=sigma_min, sigma_max=sigma_max)
        plan, Y, end, red = self._solve_plan(who, [dict(spec, basis=basis, num_components=0, reduction=reduction)], animation,
                                             frame_start, frame_end, frame_jump, None)
        r_values = [int(r) for r in r_values]
        ops = [red[3](r) for r in r_values]
        if not ops:
            return self._diff_metrics(None, [], 0, per_frame)
        self._solve_start(who, start, len(range(frame_start, end, frame_jump)))
        self._gstep_setup(plan, dt, m)
        run = lambda rd: self._solve_run(who, plan, rd, Y, frame_start, end, frame_jump, None, K, start, m, dt, mode, acc, False)
        full, n_sel = run(None)
        self._engine.rforce_operator(red[2], ops[int(np.argmax(r_values))].V)
        out = self._diff_metrics(full, (run((red[0], red[1], op))[0] for op in ops), n_sel, per_frame)
        self.assembly_ST = {kind: red[2]}
        self.bending_indices = red[1].bending_indices
        return out

    reduced_solve_errors.__doc__ %= _SOLVE_SCOPE

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
