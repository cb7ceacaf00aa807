"""``ResidentDynamics`` -- what ``posSnapshots`` offers beyond the reference's class: the pieces of the reference's
projective-dynamics solver (Simulators.py) evaluated on the device for the frames of the resident animation -- constraint
projections, constraint forces, their DEIM reduction, the global step, the solver's iterations and its time steps, with the choice of the global step's solver and
of how many kinds a solve may reduce, the positional constraints (pins) of every such call, the global step in a position
subspace q = o + U z, roll-outs whose state lives in z, and the external forces and the floor of the time steps.
A public call checks its arguments into the named records below before the engine is touched; the helpers take the records.
"""
import collections

import numpy as np

from . import projections as _proj
from . import reduced as _red


class Frames(collections.namedtuple("Frames", "which start end jump Y")):
    """The frames range(start, end, jump) of the training tensor (``which`` 0) or of the held-out animation ``Y`` (``which`` 1)."""
    __slots__ = ()

    @property
    def n_sel(self):
        return len(range(self.start, self.end, self.jump))

    def args(self, host):
        """The seven leading arguments of the engine's ``*_run`` calls."""
        return (self.which, self.start, self.end, self.jump, host.invMassL, host._standarize, host.pre_scale_factor)

    def upload(self, host):
        """The held-out animation onto the device, transformed like the training tensor."""
        if self.Y is not None:
            host._engine.heldout_upload(self.Y, host.massL, host._standarize, host.pre_scale_factor)


# One element kind of a call: its rest set-up (projections.ProjectionSetup), S^T (CSR, weighted by wi) and the strain clamp.
Term = collections.namedtuple("Term", "kind setup St sigma_min sigma_max wi")
# The explicit state s_f = x_f (+ x_f - x_{f-1}, ``mode`` 1) + ``acc`` = dt^2 g and its inertia term ``diag`` = masses / dt^2.
Explicit = collections.namedtuple("Explicit", "mode acc diag masses dt")
# A reduced kind of a solve: its ``index`` in the plan, the full set-up and S^T, ``operator``: r -> reduced.ReducedOperator,
# and ``op``: the operator in use (None until one is chosen), the engine's ``rforce_operator`` holding at least its columns.
# A solve carries a tuple of them, in list order; with more than one (``set_reduced_kinds``) the i-th lives on the engine's bank i.
Reduced = collections.namedtuple("Reduced", "index setup St operator op")
# One kind with a basis: what ``reduced_constraint_forces`` and the ``reduced_*_errors`` methods check their arguments into.
ReducedPlan = collections.namedtuple("ReducedPlan", "term frames operator")
# The positional constraints of a call (the reference's PositionalConstraint, one per vertex): ``vertices`` (P,) int64, ``wi`` (P,),
# ``p0`` (P, 3) the targets at rest, ``shift`` None (fixed) or (T_s, 3) / (T_s, P, 3) (p0 + shift[row]), ``start``: the row of
# frame 0's first step, and ``St``: the (N, P) CSR with wi_i at (v_i, i).  Not a kind: no slot, no reduction, no dependence on q.
Pins = collections.namedtuple("Pins", "vertices wi p0 shift start St")
# The external forces of a call (the reference's fext without gravity): ``table`` (3 N,) (constant) or (T_s, 3 N), the displacements
# fa = dt^2 force / mass, dense, row 3 v + d; ``start``: the row of frame 0's first step.
Forces = collections.namedtuple("Forces", "table start")
# The floor of a call (the reference's resolve_collision): coordinate ``axis`` of the explicit state is kept >= ``height``.
Floor = collections.namedtuple("Floor", "height axis")
# What a time step takes from outside: ``forces`` and ``floor``, either None (not both: that is ext = None).
External = collections.namedtuple("External", "forces floor")
FORCE_TABLE_BYTES = 2 ** 31       # the largest force table the device holds


class ResidentDynamics(object):
    """Mixin of ``posSnapshots``.  Reads from the host object: ``_engine``, ``_comm``, ``nVerts``, ``frs``, ``verts``, ``tris``,
    ``test_verts``, ``mass``, ``massL``, ``invMassL``, ``_standarize``, ``pre_scale_factor``, ``mean`` and ``snapTensor``.
    Leaves: ``assembly_ST``, ``bending_indices``, ``global_matrix``, ``global_solve_residual`` and, under the slab solver
    (``set_global_solver``), ``global_solve_slabs`` = (slabs, vertices of the largest); under the position subspace,
    ``global_solve_subspace`` = r."""

    # ------------------------------------------------------------------ the records of a call
    def _frames(self, animation, frame_start, frame_end, frame_jump):
        """The checked ``Frames`` of a public call; ``frame_end`` None: the animation's last frame."""
        if isinstance(animation, str) and animation not in ("train", "test"):
            raise ValueError("animation must be 'train', 'test' or an (F', N, 3) array, not %r" % (animation,))
        train = isinstance(animation, str) and animation == "train"
        Y, F = None, self.frs
        if not train:
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
        return Frames(0 if train else 1, frame_start, frame_end, frame_jump, Y)

    def _setup(self, kind, elements, rest_positions, sigma_min, sigma_max):
        """The checks of one element kind and its rest set-up."""
        if kind not in _proj.KINDS:
            raise ValueError("unknown projection kind %r: one of %s" % (kind, ", ".join(sorted(_proj.KINDS))))
        if self._comm.multi:
            raise NotImplementedError("constraint_projections on several ranks: elements straddle the vertex shards and no "
                                      "halo of positions is built")
        if not sigma_min <= sigma_max:
            raise ValueError("sigma_min %r > sigma_max %r" % (sigma_min, sigma_max))
        if elements is None:
            if kind != "verts_bending" or self.tris is None:
                raise ValueError("%s: no elements given%s" % (kind, " and the snapshots have no triangles" if kind == "verts_bending" else ""))
            elements = self.tris
        if rest_positions is None:
            rest_positions = self._rest()
        rest = np.asarray(rest_positions, dtype=np.float64)
        if rest.shape != (self.nVerts, 3):
            raise ValueError("rest positions of shape %s: (%d, 3) expected" % (rest.shape, self.nVerts))
        return _proj.build_setup(kind, elements, rest)

    def _rest(self):
        """The rest positions a call takes when none are given: frame 0 of the world-space input."""
        if self.verts is not None:
            return self.verts[0]
        # an adopted device tensor: frame 0 back in world space
        return self.snapTensor[0] / self.pre_scale_factor + (self.mean if self._standarize else 0.0)

    def _pins(self, who, pins, frames=None, steps=1):
        """The checked ``Pins`` of a public call (None for None), before anything touches the device.  With ``frames``: every row
        of the shift that ``steps`` time steps from those frames read must exist."""
        if pins is None:
            return None
        known = ("vertices", "wi", "positions", "shift", "shift_start")
        if not isinstance(pins, dict) or "vertices" not in pins or "wi" not in pins:
            raise ValueError("%s: pins must be a dict with 'vertices' and 'wi' (and %s), not %r" % (who, ", ".join(known[2:]), pins))
        extra = sorted(set(pins) - set(known))
        if extra:
            raise ValueError("%s: pins: unknown key %r (one of %s)" % (who, extra[0], ", ".join(known)))
        N = self.nVerts
        v = np.asarray(pins["vertices"])
        if v.ndim != 1 or v.size < 1 or v.dtype.kind not in "iu":
            raise ValueError("%s: pins: vertices must be a non-empty list of integers" % who)
        v = v.astype(np.int64)
        if v.min() < 0 or v.max() >= N:
            raise ValueError("%s: pins: vertex %d is outside 0 .. %d" % (who, int(v[(v < 0) | (v >= N)][0]), N - 1))
        if np.unique(v).size != v.size:
            raise ValueError("%s: pins: a vertex is pinned twice" % who)
        P = v.size
        try:
            w = np.asarray(pins["wi"], dtype=np.float64)
        except (TypeError, ValueError):
            w = np.full(1, np.nan)
        if w.shape not in ((), (P,)):
            raise ValueError("%s: pins: wi of shape %s: a scalar or (%d,) expected" % (who, w.shape, P))
        if not np.isfinite(w).all() or (w < 0.0).any():
            raise ValueError("%s: pins: every weight wi must be finite and >= 0" % who)
        w = np.ascontiguousarray(np.broadcast_to(w, (P,)))
        pos = pins.get("positions")
        p0 = np.asarray(self._rest(), dtype=np.float64)[v] if pos is None else np.asarray(pos, dtype=np.float64)
        if p0.shape != (P, 3) or not np.isfinite(p0).all():
            raise ValueError("%s: pins: positions of shape %s: finite (%d, 3) expected" % (who, p0.shape, P))
        shift = pins.get("shift")
        if shift is not None:
            shift = np.ascontiguousarray(shift, dtype=np.float64)
            if shift.ndim not in (2, 3) or shift.shape[0] < 1 or shift.shape[1:] not in ((3,), (P, 3)) or not np.isfinite(shift).all():
                raise ValueError("%s: pins: shift of shape %s: finite (T_s, 3) or (T_s, %d, 3) expected" % (who, shift.shape, P))
        start = pins.get("shift_start", 0)
        if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or start < 0:
            raise ValueError("%s: pins: shift_start %r: a non-negative integer" % (who, start))
        out = Pins(v, w, np.ascontiguousarray(p0), shift, int(start), _proj.pins_ST(v, w, N))
        if frames is not None and shift is not None:
            last = out.start + range(frames.start, frames.end, frames.jump)[-1] + steps - 1
            if last >= shift.shape[0]:
                raise ValueError("%s: pins: row %d of shift is needed (shift_start %d, last frame %d, %d step%s), it has %d"
                                 % (who, last, out.start, last - out.start - steps + 1, steps, "" if steps == 1 else "s", shift.shape[0]))
        return out

    def _external(self, who, forces, floor, ex, frames, steps=1):
        """The checked ``External`` of a public call (None when both are None), before anything touches the device: ``Forces``
        with the displacement table fa = dt^2 (force / masses) in f64, the reference's order (Simulators.py:494-495), the
        ``vertices`` form expanded to dense, every row that ``steps`` time steps from ``frames`` read present; ``Floor``."""
        if forces is None and floor is None:
            return None
        N = self.nVerts
        F = None
        if forces is not None:
            known = ("force", "vertices", "start")
            if not isinstance(forces, dict) or "force" not in forces:
                raise ValueError("%s: forces must be a dict with 'force' (and %s), not %r" % (who, ", ".join(known[1:]), forces))
            extra = sorted(set(forces) - set(known))
            if extra:
                raise ValueError("%s: forces: unknown key %r (one of %s)" % (who, extra[0], ", ".join(known)))
            rows = N
            v = forces.get("vertices")
            if v is not None:
                v = np.asarray(v)
                if v.ndim != 1 or v.size < 1 or v.dtype.kind not in "iu":
                    raise ValueError("%s: forces: vertices must be a non-empty list of integers" % who)
                v = v.astype(np.int64)
                if v.min() < 0 or v.max() >= N:
                    raise ValueError("%s: forces: vertex %d is outside 0 .. %d" % (who, int(v[(v < 0) | (v >= N)][0]), N - 1))
                if np.unique(v).size != v.size:
                    raise ValueError("%s: forces: a vertex is listed twice" % who)
                rows = v.size
            try:
                f = np.asarray(forces["force"], dtype=np.float64)
            except (TypeError, ValueError):
                f = np.full(1, np.nan)
            if f.ndim not in (2, 3) or f.shape[0] < 1 or f.shape[-2:] != (rows, 3) or not np.isfinite(f).all():
                raise ValueError("%s: forces: force of shape %s: finite (%d, 3) or (T_s, %d, 3) expected" % (who, f.shape, rows, rows))
            start = forces.get("start", 0)
            if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or start < 0:
                raise ValueError("%s: forces: start %r: a non-negative integer" % (who, start))
            if f.ndim == 3:
                last = int(start) + range(frames.start, frames.end, frames.jump)[-1] + steps - 1
                if last >= f.shape[0]:
                    raise ValueError("%s: forces: row %d of force is needed (start %d, last frame %d, %d step%s), it has %d"
                                     % (who, last, start, last - start - steps + 1, steps, "" if steps == 1 else "s", f.shape[0]))
            nbytes = (f.shape[0] if f.ndim == 3 else 1) * 3 * N * 8
            if nbytes > FORCE_TABLE_BYTES:
                raise ValueError("%s: forces: the dense table of %d rows x %d doubles takes %d bytes on the device, more than the %d it may "
                                 "(fewer rows per call: continue with state= and start raised)" % (who, nbytes // (24 * N), 3 * N, nbytes, FORCE_TABLE_BYTES))
            if ex.masses.shape != (N,) or not (ex.masses > 0.0).all():
                raise ValueError("%s: forces: masses of shape %s: %d positive numbers expected" % (who, ex.masses.shape, N))
            if v is not None:
                dense = np.zeros(f.shape[:-2] + (N, 3))
                dense[..., v, :] = f
                f = dense
            fa = (ex.dt * ex.dt) * (f / ex.masses[:, None])
            if not np.isfinite(fa).all():
                raise ValueError("%s: forces: dt^2 force / mass is not finite" % who)
            F = Forces(np.ascontiguousarray(fa.reshape(fa.shape[:-2] + (3 * N,))), int(start))
        L = None
        if floor is not None:
            known = ("height", "axis")
            if not isinstance(floor, dict) or "height" not in floor:
                raise ValueError("%s: floor must be a dict with 'height' (and axis), not %r" % (who, floor))
            extra = sorted(set(floor) - set(known))
            if extra:
                raise ValueError("%s: floor: unknown key %r (one of %s)" % (who, extra[0], ", ".join(known)))
            try:
                h = float(floor["height"])
            except (TypeError, ValueError):
                h = float("nan")
            if not np.isfinite(h):
                raise ValueError("%s: floor: height %r: a finite number" % (who, floor["height"]))
            axis = floor.get("axis", 1)
            if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)) or axis not in (0, 1, 2):
                raise ValueError("%s: floor: axis %r: 0, 1 or 2" % (who, axis))
            L = Floor(h, int(axis))
        return External(F, L)

    def _ext_set(self, ext):
        self._engine.ext_set(None if ext.forces is None else ext.forces.table, None if ext.floor is None else tuple(ext.floor))

    def _ext_bind(self, ext):
        self._engine.pdsolve_external(0 if ext.forces is None else ext.forces.start)

    def _plan(self, kinds, chunk_frames=None):
        """The checks of ``constraint_forces`` on its kinds, in its order: one ``Term`` per kind."""
        if not isinstance(kinds, (list, tuple)) or len(kinds) == 0:
            raise ValueError("constraint_forces: kinds must be a non-empty list of dicts, not %r" % (kinds,))
        if chunk_frames is not None and (int(chunk_frames) != chunk_frames or chunk_frames < 1):
            raise ValueError("constraint_forces: chunk_frames %r: a positive number of frames or None" % (chunk_frames,))
        known = ("kind", "elements", "wi", "rest_positions", "sigma_min", "sigma_max")
        plan = []
        for spec in kinds:
            if not isinstance(spec, dict) or "kind" not in spec:
                raise ValueError("constraint_forces: every entry of kinds is a dict with a 'kind', not %r" % (spec,))
            extra = sorted(set(spec) - set(known))
            if extra:
                raise ValueError("constraint_forces: unknown key %r (one of %s)" % (extra[0], ", ".join(known)))
            kind, smin, smax, wi = spec["kind"], spec.get("sigma_min", 1.0), spec.get("sigma_max", 1.0), spec.get("wi", 1.0)
            setup = self._setup(kind, spec.get("elements"), spec.get("rest_positions"), smin, smax)
            if any(kind == t.kind for t in plan):
                raise ValueError("constraint_forces: kind %r is listed twice" % (kind,))
            plan.append(Term(kind, setup, _proj.assembly_ST(setup, self.nVerts, wi), smin, smax, wi))
        return plan

    @staticmethod
    def _operator(term, basis, reduction):
        """r -> ``reduced.ReducedOperator`` of the basis for the kind of ``term``."""
        if reduction not in _red.REDUCTIONS:
            raise ValueError("unknown reduction %r: one of %s" % (reduction, ", ".join(sorted(_red.REDUCTIONS))))
        data = _red.load_basis(basis)
        return lambda r: _red.reduced_operator(data["components"], data["interpol_alphas"], data["Pt"], data["interpol_alpha_ranges"],
                                               r, term.setup.p, reduction, n_elements=term.setup.n_elem,
                                               verts_bending=term.kind == "verts_bending")

    def _reduced_plan(self, spec, basis, reduction, frames):
        """The ``ReducedPlan`` of one kind (``spec``: a dict of ``constraint_forces``) with a basis."""
        term, = self._plan([spec])
        return ReducedPlan(term, frames, self._operator(term, basis, reduction))

    def _explicit(self, who, dt, velocity, gravity, masses):
        """The one-rank refusal and the checks of the explicit state's arguments: ``Explicit``."""
        self._one_rank(who)
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
        masses = self._masses(masses)
        return Explicit(1 if velocity == "difference" else 0, h * h * g, masses * (1.0 / (h * h)), masses, dt)

    def _masses(self, masses):
        masses = self.mass if masses is None else masses
        if masses is None:
            raise ValueError("no vertex masses: the snapshots were built without mass weighting, pass masses=")
        return np.asarray(masses, dtype=np.float64)

    def _one_rank(self, who):
        if self._comm.multi:
            raise NotImplementedError("%s on several ranks: the system matrix couples the vertex shards and no distributed "
                                      "solve is built" % who)

    # ------------------------------------------------------------------ what every run shares
    def _alloc(self, frames, rows=None):
        """The result of a call: a caller-owned device tensor (F', rows, 3), rows = N by default."""
        import torch
        return torch.empty((frames.n_sel, self.nVerts if rows is None else rows, 3), dtype=torch.float64,
                           device="cuda:%d" % self._engine.device_id)

    def _leave(self, terms, pins=None):
        self.assembly_ST = {t.kind: t.St for t in terms}
        if pins is not None:
            self.assembly_ST["positional"] = pins.St
        self.bending_indices = next((t.setup.bending_indices for t in terms if t.kind == "verts_bending"), None)

    def _cforce_run(self, plan, frames, chunk_frames, pins=None):
        """``constraint_forces`` for a plan of ``_plan``; ``pins``: their term is added behind the kinds'."""
        frames.upload(self)
        out = self._alloc(frames)
        for i, t in enumerate(plan):
            self._engine.cproj_setup(t.setup)
            self._engine.cforce_run(*frames.args(self), t.sigma_min, t.sigma_max, t.St, i > 0,
                                    0 if chunk_frames is None else int(chunk_frames), out.data_ptr())
        if pins is not None:
            self._pins_set(pins)
            self._engine.pins_term(frames.start, frames.end, frames.jump, pins.start, True, out.data_ptr())
        self._leave(plan, pins)
        return out

    def _pins_set(self, pins):
        self._engine.pins_set(pins.vertices, pins.wi, pins.p0, pins.shift)

    def _rforce_term(self, term, op, frames):
        """One reduced term with the operator of the engine: only the sampled elements are set up and projected."""
        self._engine.cproj_setup(_proj.subset_setup(term.setup, op.elements))
        self._engine.rforce_solver(op.H, op.local_rows)
        out = self._alloc(frames)
        self._engine.rforce_run(*frames.args(self), term.sigma_min, term.sigma_max, False, out.data_ptr())
        return out

    def _step(self, b, ex, frames, pins=None):
        """A^-1 (b + M / dt^2 s) of the selected frames; the inertia term is added onto ``b``.  With ``pins`` the constant of a
        solve is formed first, as a solve forms it: c = fl(fl(M / dt^2 s) + pin term), then b = fl(b + c)."""
        if pins is None:
            self._engine.gstep_inertia(*frames.args(self), ex.diag, ex.mode, ex.acc, b.data_ptr())
            return self.global_solve(b)
        c = self._alloc(frames)
        self._pins_set(pins)
        self._engine.pins_term(frames.start, frames.end, frames.jump, pins.start, False, c.data_ptr())
        self._engine.gstep_inertia(*frames.args(self), ex.diag, ex.mode, ex.acc, c.data_ptr())
        self._engine.fm_add(b.data_ptr(), c.data_ptr(), b.numel())
        return self.global_solve(b)

    def _errors(self, plan, r_values, per_frame, full, reduced, hyper=None):
        """The body of the ``reduced_*_errors`` methods for a ``ReducedPlan``: ``full()`` makes the full device tensor, once;
        ``reduced(op)`` the one of a ``ReducedOperator``, S^T V of the largest r on the device by then -- and with ``hyper``
        A^-1 S^T V of that r, formed once behind it."""
        r_values = [int(r) for r in r_values]
        ops = [plan.operator(r) for r in r_values]
        if not ops:
            return self._diff_metrics(None, [], 0, per_frame)
        ref = full()
        self._engine.rforce_operator(plan.term.St, ops[int(np.argmax(r_values))].V)
        if hyper is not None:
            self._engine.hyper_operator()
        out = self._diff_metrics(ref, (reduced(op) for op in ops), plan.frames.n_sel, per_frame)
        self._leave([plan.term])
        return out

    @staticmethod
    def _metrics(sums, m, norms, pf):
        """``(fro, max, rel_x, rel_y, rel_z, per frame or None)`` from what ``force_diff`` / ``gsub_expand_diff`` return."""
        with np.errstate(divide='ignore', invalid='ignore'):
            rel = [float(np.sqrt(sums[d]) / np.sqrt(norms[d])) for d in range(3)]
            return (float(np.sqrt(sums.sum())), float(m / norms[3]), rel[0], rel[1], rel[2],
                    None if pf is None else np.sqrt(pf[:, 0]) / np.sqrt(pf[:, 1]))

    def _diff_metrics(self, full, others, n_sel, per_frame):
        """The reference's three metrics (constraintsComponents.py:524-556) of ``(full, t)`` for every device tensor ``t`` of
        ``others`` (made one at a time), through ``asb_force_diff``: the lists ``fro, max, rel_x, rel_y, rel_z`` and, with
        ``per_frame``, the (len(others), F') array of |full[f] - t[f]| / |full[f]|."""
        fro, mx, rel, frames = [], [], [[], [], []], []
        for t in others:
            one = self._metrics(*self._engine.force_diff(full.data_ptr(), t.data_ptr(), n_sel, self.nVerts, per_frame))
            fro.append(one[0])
            mx.append(one[1])
            for d in range(3):
                rel[d].append(one[2 + d])
            if per_frame:
                frames.append(one[5])
        out = (fro, mx, rel[0], rel[1], rel[2])
        return out + (np.array(frames).reshape(len(fro), -1) if fro else np.zeros((0, 0)),) if per_frame else out

    # ------------------------------------------------------------------ constraint projections and forces of the animation
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
        frames = self._frames(animation, frame_start, frame_end, frame_jump)
        setup = self._setup(kind, elements, rest_positions, sigma_min, sigma_max)
        St = None if wi is None else _proj.assembly_ST(setup, self.nVerts, wi)
        frames.upload(self)
        self._engine.cproj_setup(setup)
        out = self._alloc(frames, setup.rows)
        self._engine.cproj_run(*frames.args(self), sigma_min, sigma_max, out.data_ptr())
        self.bending_indices = setup.bending_indices
        if St is not None:
            self.assembly_ST = {kind: St}
        return out, frames.n_sel, setup.rows

    def constraint_forces(self, kinds, animation="train", frame_start=0, frame_end=None, frame_jump=1, chunk_frames=None, pins=None):
        """Extra (not in the reference's class): the constraint term of the global step's right-hand side,
        b[f] = sum_k S_k^T p_k(q_f) (``get_sum_ST_p``, Simulators.py:643-724), for the frames
        range(frame_start, frame_end, frame_jump) of the resident animation -- on the device, the projections p never formed
        at full size and never downloaded.

        ``kinds``: a non-empty list of dicts ``{"kind", "elements", "wi": 1.0, "rest_positions": None, "sigma_min": 1.0,
        "sigma_max": 1.0}`` with the meanings of ``constraint_projections``; a kind may be listed once.  The terms are added
        in list order.  ``chunk_frames``: frames per pass of the device (rounded up to a multiple of 16; None: as many as a
        256 MB scratch holds), which bounds the scratch and changes no bit of the result.

        ``pins``: None or the positional constraints of the reference (``PositionalConstraint``,
        Constraint_projections.py:77-113; ``project_to_positional_constraint_manifold``, Simulators.py:401-413), a dict
        ``{"vertices": (P,) distinct integers, "wi": a scalar or (P,) >= 0, "positions": None or (P, 3), "shift": None or
        (T_s, 3) or (T_s, P, 3), "shift_start": 0}``: vertex v_i is held at positions[i] (None: the rest positions at those
        vertices, the reference's ``p0``) + shift[row] (None: ``motion_type='fixed'``, else ``'user_defined'``) with weight
        wi_i, which adds wi_i (positions[i] + shift[row]) to b at v_i.  The row of selected frame f is shift_start + f -- the
        reference indexes with its step counter, which is f when it steps from the state of frame f; a row beyond T_s is a
        ValueError (the reference: IndexError).  Pins are not a kind: they take no slot and cannot be reduced.

        Returns ``(tensor, F')``: a ``torch.float64`` device tensor (F', N, 3) in world space, allocated here through torch
        and owned by the caller -- the layout ``posSnapshots.from_device`` adopts.  Leaves ``self.assembly_ST`` (kind -> CSR;
        with ``pins`` also "positional", the (N, P) CSR ``projections.pins_ST``) and ``self.bending_indices``.  One rank only."""
        frames = self._frames(animation, frame_start, frame_end, frame_jump)
        pins = self._pins("constraint_forces", pins, frames)
        return self._cforce_run(self._plan(kinds, chunk_frames), frames, chunk_frames, pins), frames.n_sel

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
        spec = dict(kind=kind, elements=elements, wi=wi, rest_positions=rest_positions, sigma_min=sigma_min, sigma_max=sigma_max)
        plan = self._reduced_plan(spec, basis, reduction, self._frames(animation, frame_start, frame_end, frame_jump))
        op = plan.operator(num_components)
        plan.frames.upload(self)
        self._engine.rforce_operator(plan.term.St, op.V)
        out = self._rforce_term(plan.term, op, plan.frames)
        self._leave([plan.term])
        return out, plan.frames.n_sel

    def reduced_force_errors(self, kind, basis, r_values, elements=None, wi=1.0, reduction="deim_pod", rest_positions=None,
                             sigma_min=1.0, sigma_max=1.0, animation="train", frame_start=0, frame_end=None, frame_jump=1,
                             per_frame=False):
        """Extra (not in the reference): how wrong the forces of the reduced simulation are -- for every r of ``r_values`` the
        reference's ``frobenius_error``, ``max_pointwise_error`` and ``relative_error_per_component``
        (constraintsComponents.py:524-556) of ``(b, b~_r)``, b the full term of ``constraint_forces`` for this kind and b~_r
        ``reduced_constraint_forces`` with r components, as five lists ``fro, max, rel_x, rel_y, rel_z``; with ``per_frame``
        a sixth value, the (len(r_values), F') array of |b[f] - b~_r[f]| / |b[f]| (Frobenius norms of the frame).  Arguments as
        ``reduced_constraint_forces``.  The full term is computed once, S^T V once for the largest r (prefixes of its
        columns serve the others); both tensors stay on the device and are compared there (asb_force_diff).  The sweep keeps
        its one kind whatever ``set_reduced_kinds`` allows: multi-kind sweeps are out of scope."""
        spec = dict(kind=kind, elements=elements, wi=wi, rest_positions=rest_positions, sigma_min=sigma_min, sigma_max=sigma_max)
        plan = self._reduced_plan(spec, basis, reduction, self._frames(animation, frame_start, frame_end, frame_jump))
        return self._errors(plan, r_values, per_frame, lambda: self._cforce_run([plan.term], plan.frames, None),
                            lambda op: self._rforce_term(plan.term, op, plan.frames))

    # ------------------------------------------------------------------ the global step of projective dynamics
    def global_solve_setup(self, kinds, dt, masses=None, pins=None):
        """Extra (not in the reference's class): prepares the global step of the reference's projective-dynamics solver,
        ``prepare_global_matrix`` (Simulators.py:117-145), for this mesh: A = M / dt^2 + sum_i w_i S_i^T S_i is assembled on
        the host from the rest tables (``projections.global_matrix``: one N x N matrix serves the three coordinates) and
        inverted once on the device, where A^-1 stays until the next set-up.

        ``kinds``: the list of dicts of ``constraint_forces`` (same checks).  ``dt``: the time step h.  ``masses`` (N,): None
        takes the vertex masses the snapshots were mass-weighted with.  Leaves ``self.global_matrix`` (CSR) and
        ``self.global_solve_residual`` = max |A (A^-1 1) - 1| as the device computed it.  Cost: the host assembly and symmetry
        check, and on the device a dense N x N inversion (N^3 flop, 8 N^2 bytes); a set-up whose matrix equals the one the
        device already holds keeps that inverse.  N <= 46 000, one rank only.  Under ``set_global_solver("slab")`` the matrix is
        factorised over breadth-first slabs instead (no limit on N but memory) and ``self.global_solve_slabs`` is left too.
        ``pins`` (the dict of ``constraint_forces``): every wi_i is added to A at (v_i, v_i), as the reference's triplets are
        (Constraint_projections.py:106-113); only ``vertices`` and ``wi`` matter here."""
        self._one_rank("global_solve_setup")
        pins = self._pins("global_solve_setup", pins)
        self._matrix(self._plan(kinds), self._masses(masses), dt, pins)

    def set_global_solver(self, kind="inverse", slab_target=None, basis=None, num_components=None, origin=None):
        """Extra: how every later call of this object applies A^-1 -- ``global_solve``, ``global_step``, ``solve_frames``,
        ``simulate_frames`` and the four ``reduced_*_errors`` sweeps that solve.

        ``kind`` "inverse" (the default): the explicit dense inverse of ``global_solve_setup``, N <= 46 000.  "slab": A is
        ordered by breadth-first level sets of its own graph grouped into slabs of at least ``slab_target`` vertices
        (``projections.slab_plan``), factorised block-tridiagonally on the device and applied by a forward and a backward
        sweep over the slabs (csrc/asb_gslab.hip): no limit on N but memory -- the factor holds the sum of the
        squared slab sizes in doubles, a solve one work matrix of N x 3 F' more.  ``slab_target``: None takes
        ``projections.SLAB_TARGET`` (256); only with "slab".  Results of the two solvers agree to rounding (64 eps kappa(A)
        max |q| each), not to the bit; under either, repeats, frame sub-ranges and chunk widths give identical bits.
        Out of scope under "slab": ``history=True`` of ``solve_frames`` (ValueError).  The arguments are checked before the
        device is touched; the device's solver is replaced by the next call that needs the matrix.

        "subspace": the global step in a POSITION subspace q = o + U z, the reference's ``reduced_position`` branch
        (Simulators.py:38-41, :144-155, which it leaves unimplemented): per coordinate the Galerkin step
        q_d = o_d + U_d (U_d^T A U_d)^-1 U_d^T (rhs_d - A o_d) replaces A^-1 rhs_d everywhere (csrc/asb_gsub.hip).
        This is no approximation of A^-1 to rounding: results differ from the other two solvers by the part of the step outside
        the subspace.  ``basis``: a world-space array (K, N, 3), the path of a ``.npy`` holding one, or a ``posComponents`` (its
        ``comps``, taken back to world space with its snapshots' ``invMassL`` where they live in the mass-weighted space); only
        the span matters (``projections.subspace_basis`` orthonormalises per coordinate and refuses a rank-deficient basis).
        ``num_components`` = r: the first r components (None: all K).  ``origin``: None takes the rest positions (frame 0 of the
        world-space input, resolved when the matrix is set up) or an (N, 3) array.  The three are for "subspace" only.  Pins need
        nothing new: their weights are in A, their term in the right-hand side.  Held on the device: 3 x 3 r N doubles and
        3 r F' more in a solve.  Out of scope under "subspace": ``history=True`` (ValueError),
        an M-orthogonal basis, several ranks.  (A roll-out whose state lives in z is ``simulate_subspace``, the sweep over r along such roll-outs ``subspace_rollout_errors``.)  Limits under "subspace": r <= min(N, 8192) (ValueError here, before the device is
        touched); with ``hyper`` a reduced kind of at most 21 845 basis vectors (the engine refuses more; 65 532 under the other
        two solvers: the operator's rows go through one grid dimension).  Leaves ``self.global_solve_subspace`` = r after the next set-up."""
        if kind not in ("inverse", "slab", "subspace"):
            raise ValueError("set_global_solver: kind must be 'inverse' or 'slab', not %r (or 'subspace', with a basis)" % (kind,))
        if kind != "subspace":
            for name, given in (("basis", basis), ("num_components", num_components), ("origin", origin)):
                if given is not None:
                    raise ValueError("set_global_solver: %s is for kind='subspace' only" % name)
        if slab_target is not None:
            if kind != "slab":
                raise ValueError("set_global_solver: slab_target is for kind='slab' only")
            try:
                t = int(slab_target)
            except (TypeError, ValueError):
                t = 0
            if t != slab_target or isinstance(slab_target, bool) or t < 1:
                raise ValueError("set_global_solver: slab_target %r: a positive number of vertices per slab or None" % (slab_target,))
            slab_target = t
        subspace = None
        if kind == "subspace":
            subspace = self._subspace_args("set_global_solver", basis, num_components, origin)
        self._global_solver, self._global_subspace = (kind, slab_target), subspace

    def _subspace_args(self, who, basis, num_components, origin):
        """The checked ``(Qt, origin or None)`` of a position subspace: Qt (3, r, N) from ``projections.subspace_basis``."""
        if basis is None:
            raise ValueError("%s: kind='subspace' needs a basis: a (K, N, 3) array, the path of a .npy or a posComponents" % who)
        try:
            Qt = _proj.subspace_basis(basis, num_components, self.nVerts)
        except ValueError as e:
            raise ValueError("%s: %s" % (who, e))
        if Qt.shape[1] > _proj.SUBSPACE_MAX_R:
            raise ValueError("%s: %d components: the engine holds at most %d per coordinate" % (who, Qt.shape[1], _proj.SUBSPACE_MAX_R))
        if origin is not None:
            try:
                origin = np.array(origin, dtype=np.float64)
            except (TypeError, ValueError):
                origin = np.zeros(0)
            if origin.shape != (self.nVerts, 3) or not np.isfinite(origin).all():
                raise ValueError("%s: origin of shape %s: a finite (%d, 3) array or None expected" % (who, origin.shape, self.nVerts))
        return Qt, origin

    def _slab_solver(self):
        """None under the explicit inverse and under the position subspace, else the slab target in force."""
        kind, target = getattr(self, "_global_solver", ("inverse", None))
        return None if kind != "slab" else (_proj.SLAB_TARGET if target is None else target)

    def _subspace_solver(self):
        """None unless the position subspace is selected, else its ``(Qt, origin or None)``."""
        return getattr(self, "_global_subspace", None) if getattr(self, "_global_solver", ("inverse", None))[0] == "subspace" else None

    def _matrix(self, plan, masses, dt, pins=None):
        """A of the plan (and the pins' weights on its diagonal), inverted (or, under the slab solver, factorised) on the device
        unless the device holds that very matrix."""
        if pins is None:
            A = _proj.global_matrix([(t.setup, t.wi) for t in plan], self.nVerts, masses, dt)
        else:
            A = _proj.global_matrix([(t.setup, t.wi) for t in plan], self.nVerts, masses, dt, (pins.vertices, pins.wi))
        self.global_matrix, self.global_solve_residual = None, None
        sub = self._subspace_solver()
        if sub is not None:
            self.global_solve_subspace = None
            Qt, origin = sub
            origin = np.ascontiguousarray(self._rest() if origin is None else origin, dtype=np.float64)
            resid = self._engine.gsub_held(A, Qt, origin)
            if resid is None:
                resid = self._engine.gsub_setup(A, Qt, origin)
            self.global_matrix, self.global_solve_residual, self.global_solve_subspace = A, resid, int(Qt.shape[1])
            return
        target = self._slab_solver()
        if target is not None:
            self.global_solve_slabs = None
            sp = _proj.slab_plan(A, target)
            held = self._engine.gslab_held(A, sp)
            if held is None:
                held = self._engine.gslab_setup(A, sp)
            self.global_matrix, self.global_solve_residual = A, held[0]
            self.global_solve_slabs = (len(sp.slab_ptr) - 1, int(np.diff(sp.slab_ptr).max()))
            return
        resid = self._engine.gstep_held(A)
        if resid is None:
            resid = self._engine.gstep_setup(A)
        self.global_matrix, self.global_solve_residual = A, resid

    def global_solve(self, rhs):
        """Extra: q = A^-1 rhs per coordinate for the matrix of the last ``global_solve_setup``.  ``rhs``: a caller-owned
        ``torch.float64`` device tensor (F', N, 3), contiguous; returns a new one of the same shape, owned by the caller.  The
        sum over the vertices is never split: a frame's result does not depend on the frames around it.  Under
        ``set_global_solver("subspace")`` the result is the AFFINE Galerkin step o' + P rhs, o' = o - P A o: a zero rhs gives o', not
        zero, and q - o always lies in span(U)."""
        self._one_rank("global_solve")
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

    def global_step(self, kinds, dt, masses=None, velocity="difference", gravity=(0.0, 0.0, 0.0), animation="train",
                    frame_start=0, frame_end=None, frame_jump=1, chunk_frames=None, pins=None):
        """Extra: one local/global iteration of the reference's solver started at every selected frame of the resident
        animation (Simulators.py:494-526 with ``num_iterations`` = 1 and q = x_f):
        Phi(x_f; s_f) = A^-1 (M / dt^2 s_f + sum_k S_k^T p_k(x_f)), on the device.

        ``kinds``, ``animation``, the frame range and ``chunk_frames``: as ``constraint_forces``; ``dt``, ``masses``: as
        ``global_solve_setup``, whose work is done here first -- the matrix is assembled on every call, the dense inversion
        is paid only when the matrix differs from the one the device holds.  ``velocity``: "zero" takes the explicit state
        s_f = x_f + dt^2 g, "difference"
        s_f = 2 x_f - x_{f-1} + dt^2 g with f - 1 the ANIMATION's previous frame whatever ``frame_jump`` is (at frame 0:
        x_0), the velocity the reference carries from step to step (:531).  ``gravity``: the acceleration g.  ``pins``: the
        positional constraints of ``constraint_forces`` -- their weights join A, their term the right-hand side, frame f with
        row shift_start + f of the shift.

        Returns ``(tensor, F')``: a ``torch.float64`` device tensor (F', N, 3) in world space, owned by the caller.  Further
        iterations are ``solve_frames``: they keep s_f fixed while q moves, which re-adopting the result with ``from_device``
        and stepping again would not.  One rank only."""
        ex = self._explicit("global_step", dt, velocity, gravity, masses)
        frames = self._frames(animation, frame_start, frame_end, frame_jump)
        pins = self._pins("global_step", pins, frames)
        plan = self._plan(kinds, chunk_frames)
        self._matrix(plan, ex.masses, ex.dt, pins)
        out = self._step(self._cforce_run(plan, frames, chunk_frames), ex, frames, pins)
        if pins is not None:
            self._leave(plan, pins)
        return out, frames.n_sel

    def reduced_global_step_errors(self, kind, basis, r_values, dt, masses=None, velocity="difference", gravity=(0.0, 0.0, 0.0),
                                   elements=None, wi=1.0, reduction="deim_pod", rest_positions=None, sigma_min=1.0,
                                   sigma_max=1.0, animation="train", frame_start=0, frame_end=None, frame_jump=1,
                                   per_frame=False, pins=None):
        """Extra: how far the reduced right-hand side moves the vertices -- ``reduced_force_errors`` one line further down the
        iteration.  Cost beside that method's: the work of ``global_solve_setup`` once, one solve plus one per r.
        For every r of ``r_values`` the three metrics of ``(q, q~_r)``: q = ``global_step`` of this kind and
        q~_r the same step with b~_r of ``reduced_constraint_forces`` in place of b (same inertia term, same A^-1).  Arguments
        as ``reduced_force_errors`` plus ``dt``, ``masses``, ``velocity``, ``gravity`` of ``global_step``; the same five lists
        ``fro, max, rel_x, rel_y, rel_z`` and, with ``per_frame``, the (len(r_values), F') array |q[f] - q~_r[f]| / |q[f]|.
        The full step is computed once; every tensor stays on the device.  The sweep keeps its one kind whatever
        ``set_reduced_kinds`` allows: multi-kind sweeps are out of scope.  ``pins`` (as ``global_step``) are part of both steps,
        unreduced."""
        ex = self._explicit("reduced_global_step_errors", dt, velocity, gravity, masses)
        spec = dict(kind=kind, elements=elements, wi=wi, rest_positions=rest_positions, sigma_min=sigma_min, sigma_max=sigma_max)
        frames = self._frames(animation, frame_start, frame_end, frame_jump)
        pins = self._pins("reduced_global_step_errors", pins, frames)
        plan = self._reduced_plan(spec, basis, reduction, frames)

        def full():
            self._matrix([plan.term], ex.masses, ex.dt, pins)
            return self._step(self._cforce_run([plan.term], plan.frames, None), ex, plan.frames, pins)
        out = self._errors(plan, r_values, per_frame, full,
                           lambda op: self._step(self._rforce_term(plan.term, op, plan.frames), ex, plan.frames, pins))
        if pins is not None and self.assembly_ST is not None:
            self.assembly_ST["positional"] = pins.St
        return out

    # ------------------------------------------------------------------ the solver's iterations
    _SOLVE_SCOPE = """Out of scope, as for ``global_step``: the self-collision passes and several ranks (external forces and the
        floor, ``resolve_collision``, are ``forces=`` / ``floor=`` of ``solve_frames`` and ``simulate_frames``; the one-shot error
        sweeps do not take them).  Every selected frame is an independent solve; further time steps from its
        result, the velocity carried along, are ``simulate_frames``.

        ``hyper`` (None, "touched" or "all"): the hyper-reduced operator A^-1 S^T V, as the reference's reduced simulator holds
        its ``projecting_mat`` (Simulators.py:157-220).  With EVERY listed kind reduced the iteration is affine in the
        coefficients, q_{k+1} = c + G coef(q_k) per coordinate with c = A^-1 M / dt^2 s_f (once per solve) and
        G = A^-1 S^T V (N x m, once per call), and coef reads q_k only at the vertices of the sampled elements: no N^2
        product is left in an iteration.  "touched": all but the last iteration run on those vertices' rows only, the last on
        all N; "all": every iteration on all N rows (for checks, and for continuing with ``start=``); both give the same
        bits.  None: the path without the operator, unchanged.  Refused with ``hyper`` (ValueError, before the device is
        touched): a kind without ``basis`` / ``num_components`` -- every kind must be reduced, which without
        ``set_reduced_kinds`` means exactly one kind --, ``history=True`` (step norms over all rows would need the whole
        iterate in every iteration) and an unknown value.  Under ``set_reduced_kinds(L)``, L > 1, up to L kinds may be
        reduced, each on an engine bank of its own; ``hyper`` then takes all of them (a list with a plain kind is refused):
        q_{k+1} = c + sum_k G_k coef_k(q_k), every coef_k from the OLD iterate -- the Jacobi update of the reference, whose
        groups' terms are summed before its one solve --, "touched" running on the union of the kinds' touched vertices
        (DESIGN.md 3.18).  Out of scope for ``hyper`` unless ``set_reduced_kinds`` raises the limit: several reduced kinds in one solve; always:
        the history, several ranks.  (No longer on this list: a reduction of the positions themselves, a basis U of q, is
        ``set_global_solver("subspace")`` and combines with ``hyper``.)  Not part of a solve, with or
        without ``hyper``: velocities carried between frames or steps -- that is ``simulate_frames``, which takes ``hyper`` too.

        ``pins``: the positional constraints of ``constraint_forces``.  Their weights join A; their term wi (p0 + shift[row]) does
        not depend on q and joins the constant M / dt^2 s_f of the solve, the row of frame f being shift_start + f.  Pins are
        not a kind: they take none of the 8 slots, do not count for ``set_reduced_kinds``, and ``hyper`` -- which needs every
        listed KIND reduced -- carries them unreduced inside c."""

    def _solve_args(self, who, dt, velocity, gravity, num_iterations, start, masses):
        """The checks of the solve's own arguments, before anything touches the device: (``Explicit``, K)."""
        ex = self._explicit(who, dt, velocity, gravity, masses)
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
        return ex, K

    def set_reduced_kinds(self, limit=1):
        """Extra: how many entries of ``kinds`` may carry ``basis`` / ``num_components`` / ``reduction`` in every later
        ``solve_frames`` and ``simulate_frames`` of this object -- the reference's reduced simulator keeps one projecting
        matrix, one set of interpolation points and one solver per constraint group (Simulators.py:49-87, :157-220) and adds
        the reduced terms of every group whose ``*_reduced`` flag is set (:415-478, :506-526).

        ``limit``: an integer 1..8 (the engine's banks).  1, the default: one reduced kind, every call, message
        and result as without this method.  L > 1: up to L reduced kinds in one solve, the i-th on the engine's bank i;
        ``hyper`` then needs EVERY listed kind reduced and runs all of them in one affine iteration on the union of their touched
        vertices.  A call with one reduced kind is the same whatever the limit.  The four ``reduced_*_errors`` sweeps keep
        their one kind.  The device buffers of a bank that a call has used stay with the engine afterwards (per bank S^T V and
        A^-1 S^T V, 24 N m bytes each), also when the limit goes back to 1.  Checked before the device is touched."""
        if isinstance(limit, bool) or not isinstance(limit, (int, np.integer)) or not 1 <= limit <= 8:
            raise ValueError("set_reduced_kinds: limit %r: an integer 1..8" % (limit,))
        self._reduced_limit = int(limit)

    def _solve_plan(self, who, kinds, chunk_frames):
        """``_plan`` of the kinds with their reduction keys taken off, and the tuple of ``Reduced`` (no operator chosen yet) of
        the entries that carry a ``basis``, in list order: at most ``set_reduced_kinds`` allows."""
        keys = ("basis", "num_components", "reduction")
        limit = getattr(self, "_reduced_limit", 1)
        if not isinstance(kinds, (list, tuple)):
            raise ValueError("%s: kinds must be a non-empty list of dicts, not %r" % (who, kinds))
        plain, red = [], []
        for i, spec in enumerate(kinds):
            if isinstance(spec, dict) and any(k in spec for k in keys):
                if "basis" not in spec or "num_components" not in spec:
                    raise ValueError("%s: a reduced kind carries both 'basis' and 'num_components'" % who)
                if len(red) >= limit and limit == 1:
                    raise ValueError("%s: a second reduced kind (%r after %r): the engine holds one reduced operator"
                                     % (who, spec.get("kind"), kinds[red[0]].get("kind")))
                if len(red) >= limit:
                    raise ValueError("%s: more than %d reduced kinds (%r): set_reduced_kinds(%d) is in force"
                                     % (who, limit, spec.get("kind"), limit))
                red.append(i)
                spec = {k: v for k, v in spec.items() if k not in keys}
            plain.append(spec)
        plan = self._plan(plain, chunk_frames)
        return plan, tuple(Reduced(i, plan[i].setup, plan[i].St,
                                   self._operator(plan[i], kinds[i]["basis"], kinds[i].get("reduction", "deim_pod")), None) for i in red)

    @staticmethod
    def _chosen(reds, kinds):
        """The ``Reduced`` of a call with the operators of their ``num_components``."""
        return tuple(r._replace(op=r.operator(int(kinds[r.index]["num_components"]))) for r in reds)

    def _with_operators(self, reds, hyper, run):
        """``run()`` behind the operators of the call: per reduced kind S^T V and, with ``hyper``, A^-1 S^T V on the device,
        once; several kinds take the engine's banks 0, 1, .. in order, and bank 0 is current again on every way out."""
        eng, multi = self._engine, len(reds) > 1
        try:
            for b, r in enumerate(reds):
                if multi:
                    eng.rforce_bank(b)
                eng.rforce_operator(r.St, r.op.V)
                if hyper is not None:
                    eng.hyper_operator()
            return run()
        finally:
            if multi:
                eng.rforce_bank(0)

    def _solve_start(self, who, start, n_sel):
        """(start code of the engine, the caller's tensor or None); a tensor is checked as ``global_solve`` checks its rhs."""
        if isinstance(start, str):
            return (0 if start == "explicit" else 1), None
        if start.device.index != self._engine.device_id:
            raise ValueError("%s: start lives on %s, the snapshots on device %d" % (who, start.device, self._engine.device_id))
        if start.dim() != 3 or tuple(start.shape) != (n_sel, self.nVerts, 3) or not start.is_contiguous():
            raise ValueError("%s: start of shape %s: a contiguous (%d, %d, 3) expected" % (who, tuple(start.shape), n_sel, self.nVerts))
        return 2, start

    def _hyper_check(self, who, hyper, kinds, history):
        """The refusals of ``hyper``, before anything touches the device."""
        if hyper is None:
            return
        if hyper not in ("touched", "all"):
            raise ValueError("%s: hyper must be None, 'touched' or 'all', not %r" % (who, hyper))
        if history:
            raise ValueError("%s: history=True with hyper=%r: the step norms run over all rows and would force the full iterate "
                             "in every iteration" % (who, hyper))
        limit = getattr(self, "_reduced_limit", 1)
        every = isinstance(kinds, (list, tuple)) and len(kinds) >= 1 and all(
            isinstance(k, dict) and "basis" in k and "num_components" in k for k in kinds)
        if limit == 1 and (not every or len(kinds) != 1):
            raise ValueError("%s: hyper=%r needs every kind reduced ('basis' and 'num_components'), and the engine holds one reduced "
                             "operator: exactly one kind, a reduced one" % (who, hyper))
        if not every:
            raise ValueError("%s: hyper=%r needs every kind reduced ('basis' and 'num_components'): up to %d of them under "
                             "set_reduced_kinds(%d), none left plain" % (who, hyper, limit, limit))

    def _solve_slots(self, plan, reds, hyper):
        """The kinds of the plan registered with the solve in progress, in order; a reduced kind as its sampled elements, with
        its solver, on its bank when there are several.  With ``hyper`` every kind is reduced and numbered in the union of
        their touched vertices, which is returned."""
        eng, multi = self._engine, len(reds) > 1
        red = {r.index: (b, r) for b, r in enumerate(reds)}
        touched, sub = self._sampled(reds, hyper)
        for i, t in enumerate(plan):
            if i in red:
                if multi:
                    eng.rforce_bank(red[i][0])
                eng.cproj_setup(sub[i])
                eng.rforce_solver(red[i][1].op.H, red[i][1].op.local_rows)
                eng.pdsolve_slot(t.sigma_min, t.sigma_max, None)
            else:
                eng.cproj_setup(t.setup)
                eng.pdsolve_slot(t.sigma_min, t.sigma_max, t.St)
        return touched

    def _sampled(self, reds, hyper):
        """(touched or None, index -> the sampled elements' set-up) of the reduced kinds; with ``hyper`` numbered in the union of
        their touched vertices."""
        multi = len(reds) > 1
        sub = {r.index: _proj.subset_setup(r.setup, r.op.elements) for r in reds}
        touched = None
        if hyper == "all":
            touched = np.arange(self.nVerts, dtype=np.int64)
            sub = {i: _proj.touched_setup(u, self.nVerts)[1] for i, u in sub.items()}
        elif hyper is not None and not multi:           # one kind: its own touched set, found once
            (i, u), = sub.items()
            touched, u = _proj.touched_setup(u)
            sub = {i: u}
        elif hyper is not None:
            touched = _proj.touched_union([sub[i] for i in sorted(sub)])
            sub = {i: _proj.touched_setup(u, into=touched)[1] for i, u in sub.items()}
        return touched, sub

    def _solve_run(self, plan, reds, frames, ex, begin, K, chunk_frames, history, hyper=None, pins=None, ext=None):
        """The solve (matrix on the device); ``reds``: the ``Reduced`` of the plan with their ``op``; ``begin``: what
        ``_solve_start`` gave.  ``hyper``: every kind is in ``reds`` and their A^-1 S^T V are on the device.  ``ext``: the
        ``External`` of the call; it is bound before the pins, whose term goes onto the inertia term it rewrites."""
        eng = self._engine
        code, start = begin
        if code == 2:
            import torch
            torch.cuda.current_stream(start.device).synchronize()   # whatever produced start is done before the engine reads it
        frames.upload(self)
        if pins is not None:
            self._pins_set(pins)
        if ext is not None:
            self._ext_set(ext)
        eng.pdsolve_begin(*frames.args(self), ex.diag, ex.mode, ex.acc, code, None if start is None else start.data_ptr())
        if ext is not None:
            self._ext_bind(ext)
        if pins is not None:
            eng.pdsolve_pins(pins.start)
        if hyper is not None:
            touched = self._solve_slots(plan, reds, hyper)
            out = self._alloc(frames)
            eng.hyper_iterate(K, None if hyper == "all" else touched, 0 if chunk_frames is None else int(chunk_frames), out.data_ptr())
            self._leave(plan, pins)
            return out, frames.n_sel
        self._solve_slots(plan, reds, None)
        out = self._alloc(frames)
        hist = eng.pdsolve_iterate(K, 0 if chunk_frames is None else int(chunk_frames), out.data_ptr(), history)
        self._leave(plan, pins)
        if history:
            with np.errstate(divide='ignore', invalid='ignore'):
                return out, frames.n_sel, np.sqrt(hist[:, :, 0]) / np.sqrt(hist[:, :, 1])
        return out, frames.n_sel

    def solve_frames(self, kinds, dt, num_iterations=10, masses=None, velocity="difference", gravity=(0.0, 0.0, 0.0), start="explicit",
                     animation="train", frame_start=0, frame_end=None, frame_jump=1, chunk_frames=None, history=False, forces=None,
                     floor=None, pins=None, hyper=None):
        """Extra: the local/global iterations of the reference's solver (Simulators.py:494-526) for every selected frame of
        the resident animation, on the device: q_0 given, q_{k+1} = A^-1 (M / dt^2 s_f + sum_i S_i^T p_i(q_k)) for
        ``num_iterations`` iterations, the explicit state s_f held fixed while q moves.  The iterate stays on the device
        between iterations in the layout the projection kernels read; the kinds' tables and S^T are uploaded once per solve.

        ``kinds``: the list of dicts of ``constraint_forces``; ONE entry -- up to L entries after ``set_reduced_kinds(L)`` --
        may also carry ``basis``, ``num_components`` and ``reduction`` (default "deim_pod") with the meanings of
        ``reduced_constraint_forces``: that kind's term is then the reduced one, as the simulator's per-group ``*_reduced``
        flags choose; the terms are added in list order.  A is always the full matrix of all listed kinds.
        ``dt``, ``masses``, ``velocity``, ``gravity``, ``animation``, the frame range and ``chunk_frames``: as ``global_step``.
        ``start``: "explicit" (q_0 = s_f, the reference's), "frame" (q_0 = x_f; one iteration is then ``global_step`` bit for
        bit) or a contiguous ``torch.float64`` device tensor (F', N, 3) -- a solve continued from an earlier result equals the
        longer solve bit for bit.  ``history``: also the (num_iterations, F') array of |q_{k+1} - q_k| / |q_{k+1}| (Frobenius
        norms of the frame); refused under ``set_global_solver("slab")``.  ``forces`` / ``floor``: as ``simulate_frames``, on the
        explicit state of the one step a solve is -- frame f reads row ``start`` + f of a per-step force --; they form the inertia
        term under every ``start``, and the first iterate too where that is the explicit state.

        Returns ``(tensor, F')`` (``(tensor, F', steps)`` with ``history``): a ``torch.float64`` device tensor (F', N, 3) in
        world space, owned by the caller.  Device memory held by the engine beside A^-1: three times the result plus the
        projections of one chunk.  %s"""
        who = "solve_frames"
        self._hyper_check(who, hyper, kinds, history)
        if history and self._slab_solver() is not None:
            raise ValueError("%s: history=True under set_global_solver('slab'): the step norms are formed by the explicit inverse's "
                             "product kernel and are out of scope for the slab solver" % who)
        if history and self._subspace_solver() is not None:
            raise ValueError("%s: history=True under set_global_solver('subspace'): the step norms are formed by the explicit inverse's "
                             "product kernel and are out of scope for the position subspace" % who)
        ex, K = self._solve_args(who, dt, velocity, gravity, num_iterations, start, masses)
        frames = self._frames(animation, frame_start, frame_end, frame_jump)
        pins = self._pins(who, pins, frames)
        ext = self._external(who, forces, floor, ex, frames)
        plan, reds = self._solve_plan(who, kinds, chunk_frames)
        begin = self._solve_start(who, start, frames.n_sel)
        reds = self._chosen(reds, kinds)
        self._matrix(plan, ex.masses, ex.dt, pins)
        return self._with_operators(reds, hyper, lambda: self._solve_run(plan, reds, frames, ex, begin, K, chunk_frames, history, hyper, pins, ext))

    solve_frames.__doc__ %= _SOLVE_SCOPE

    def reduced_solve_errors(self, kind, basis, r_values, dt, num_iterations=10, masses=None, velocity="difference",
                             gravity=(0.0, 0.0, 0.0), start="explicit", elements=None, wi=1.0, reduction="deim_pod", rest_positions=None,
                             sigma_min=1.0, sigma_max=1.0, animation="train", frame_start=0, frame_end=None, frame_jump=1,
                             per_frame=False, pins=None, hyper=None):
        """Extra: how far the DEIM-reduced simulation is from the full one after the solver's iterations -- for every r of
        ``r_values`` the three metrics of ``(q, q~_r)``, q = ``solve_frames`` of this kind and q~_r the same solve with the kind
        reduced to r components (same A^-1, same inertia term, same start).  Arguments as ``reduced_global_step_errors`` plus
        ``num_iterations`` and ``start``; the same five lists ``fro, max, rel_x, rel_y, rel_z`` and, with ``per_frame``, the
        (len(r_values), F') array |q[f] - q~_r[f]| / |q[f]|.  The full solve runs once, one reduced solve per r (S^T V once, for
        the largest r); every tensor stays on the device and is compared there.  With ``num_iterations=1, start="frame"`` these
        are the numbers of ``reduced_global_step_errors``.  With ``hyper`` the full solve still runs once as before, the per-r
        reduced solves go through the hyper-reduced path, and A^-1 S^T V is formed once, for the largest r (prefixes of its
        columns serve the others, as those of S^T V do).  The sweep keeps its one kind whatever ``set_reduced_kinds``
        allows: multi-kind sweeps are out of scope.  %s"""
        who = "reduced_solve_errors"
        self._hyper_check(who, hyper, [dict(basis=basis, num_components=0)], False)
        ex, K = self._solve_args(who, dt, velocity, gravity, num_iterations, start, masses)
        spec = dict(kind=kind, elements=elements, wi=wi, rest_positions=rest_positions, sigma_min=sigma_min, sigma_max=sigma_max)
        frames = self._frames(animation, frame_start, frame_end, frame_jump)
        pins = self._pins(who, pins, frames)
        terms, (red,) = self._solve_plan(who, [dict(spec, basis=basis, num_components=0, reduction=reduction)], None)
        begin = self._solve_start(who, start, frames.n_sel)
        run = lambda rd: self._solve_run(terms, () if rd is None else (rd,), frames, ex, begin, K, None, False, None if rd is None else hyper,
                                         pins)[0]

        def full():
            self._matrix(terms, ex.masses, ex.dt, pins)
            return run(None)
        out = self._errors(ReducedPlan(terms[0], frames, red.operator), r_values, per_frame, full,
                           lambda op: run(red._replace(op=op)), hyper)
        if pins is not None and self.assembly_ST is not None:
            self.assembly_ST["positional"] = pins.St
        return out

    reduced_solve_errors.__doc__ %= _SOLVE_SCOPE

    def subspace_solve_errors(self, kinds, basis, r_values, dt, num_iterations=10, masses=None, velocity="difference",
                              gravity=(0.0, 0.0, 0.0), start="explicit", animation="train", frame_start=0, frame_end=None, frame_jump=1,
                              chunk_frames=None, per_frame=False, pins=None, origin=None):
        """Extra: how far the POSITION-reduced solve is from the full one -- for every r of ``r_values`` the three metrics of
        ``(q, q~_r)``, q = ``solve_frames`` of these kinds under the solver selected now ("inverse" or "slab") and q~_r the same
        solve under ``set_global_solver("subspace", basis=basis, num_components=r, origin=origin)``.  Arguments as
        ``solve_frames`` without ``hyper`` and ``history`` (entries of ``kinds`` may be reduced), ``basis`` and ``origin`` as
        ``set_global_solver``; every r is checked (rank included) before the device is touched.  The same five lists
        ``fro, max, rel_x, rel_y, rel_z`` and, with ``per_frame``, the (len(r_values), F') array |q[f] - q~_r[f]| / |q[f]|.  The
        full solve runs once, one subspace set-up and solve per r; every tensor stays on the device and is compared there.  The
        solver selected for this object is the same afterwards.  (Along roll-outs: ``subspace_rollout_errors``.)"""
        who = "subspace_solve_errors"
        if self._subspace_solver() is not None:
            raise ValueError("%s: the full solve runs under 'inverse' or 'slab': set_global_solver('subspace') is in force" % who)
        subs = [self._subspace_args(who, basis, r, origin) for r in r_values]     # (r unchanged: 2.5 and True are refused)
        args = dict(masses=masses, velocity=velocity, gravity=gravity, start=start, animation=animation, frame_start=frame_start,
                    frame_end=frame_end, frame_jump=frame_jump, chunk_frames=chunk_frames, pins=pins)
        if not subs:
            return self._diff_metrics(None, [], 0, per_frame)
        full, n_sel = self.solve_frames(kinds, dt, num_iterations, **args)
        selected = (self._global_solver if hasattr(self, "_global_solver") else None, getattr(self, "_global_subspace", None))

        def under(sub):
            self._global_solver, self._global_subspace = ("subspace", None), sub
            return self.solve_frames(kinds, dt, num_iterations, **args)[0]
        try:
            return self._diff_metrics(full, (under(sub) for sub in subs), n_sel, per_frame)
        finally:
            if selected[0] is None:
                del self._global_solver
            else:
                self._global_solver = selected[0]
            self._global_subspace = selected[1]

    # ------------------------------------------------------------------ time steps: the velocity carried from step to step
    @staticmethod
    def _rollout_args(who, num_steps, record_every, state):
        """The checks of the roll-out's own arguments, before anything touches the device: (T, r or None)."""
        def count(x):
            try:
                n = int(x)
            except (TypeError, ValueError):
                return 0
            return n if n == x and not isinstance(x, bool) and n >= 1 else 0
        T = count(num_steps)
        if T < 1:
            raise ValueError("%s: num_steps %r: a positive number of time steps" % (who, num_steps))
        every = None if record_every is None else count(record_every)
        if every == 0:
            raise ValueError("%s: record_every %r: a positive number of time steps or None" % (who, record_every))
        if state is not None:
            import torch
            if not isinstance(state, (list, tuple)) or len(state) != 2 or not all(
                    isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.is_cuda for t in state):
                raise ValueError("%s: state must be a pair (q, q_prev) of torch.float64 device tensors" % who)
        return T, every

    def _rollout_state(self, who, state, n_sel):
        """The tensors of ``state`` checked as ``global_solve`` checks its rhs."""
        for t in state or ():
            if t.device.index != self._engine.device_id:
                raise ValueError("%s: state lives on %s, the snapshots on device %d" % (who, t.device, self._engine.device_id))
            if t.dim() != 3 or tuple(t.shape) != (n_sel, self.nVerts, 3) or not t.is_contiguous():
                raise ValueError("%s: state of shape %s: contiguous (%d, %d, 3) tensors expected" % (who, tuple(t.shape), n_sel, self.nVerts))

    def _rollout_run(self, plan, reds, frames, ex, state, K, T, chunk_frames, every, hyper=None, pins=None, ext=None, ext_held=False):
        """The roll-out (matrix on the device; ``reds``, ``hyper`` as ``_solve_run``): ``(q, q_prev, records or None, steps)``."""
        import torch
        eng = self._engine
        if state is not None:
            torch.cuda.current_stream(state[0].device).synchronize()    # whatever produced the state is done before the engine reads it
        frames.upload(self)
        if pins is not None:
            self._pins_set(pins)
        if ext is not None and not ext_held:        # (a sweep uploads the table once, before its roll-outs)
            self._ext_set(ext)
        if state is None:
            eng.pdsolve_begin(*frames.args(self), ex.diag, ex.mode, ex.acc, 0, None)
            eng.pdsolve_carry(None)
        else:                                       # the pair becomes (iterate, carried positions); the advance makes s_1 of them
            eng.pdsolve_begin(*frames.args(self), ex.diag, ex.mode, ex.acc, 2, state[0].data_ptr())
            eng.pdsolve_carry(state[1].data_ptr())
            eng.pdsolve_advance()
        if ext is not None:                         # on the explicit state of step 1, also the one a continuation's advance made
            self._ext_bind(ext)
        if pins is not None:                        # behind the advance of a continuation, which rewrites the inertia term
            eng.pdsolve_pins(pins.start)
        touched = self._solve_slots(plan, reds, hyper)
        steps = [] if every is None else list(range(every, T + 1, every))
        records = None
        if every is not None:
            records = torch.empty((len(steps), frames.n_sel, self.nVerts, 3), dtype=torch.float64, device="cuda:%d" % eng.device_id)
        q = records[-1] if steps and steps[-1] == T else self._alloc(frames)
        cf = 0 if chunk_frames is None else int(chunk_frames)
        for t in range(1, T + 1):
            if t > 1:
                eng.pdsolve_advance()
            out = q if t == T else (records[t // every - 1] if every is not None and t % every == 0 else None)
            ptr = None if out is None else out.data_ptr()
            if hyper is not None:
                eng.hyper_iterate(K, None if hyper == "all" else touched, cf, ptr)
            else:
                eng.pdsolve_iterate(K, cf, ptr, False)
        q_prev = self._alloc(frames)
        eng.pdsolve_positions(q_prev.data_ptr())
        self._leave(plan, pins)
        return q, q_prev, records, steps

    def simulate_frames(self, kinds, dt, num_steps, num_iterations=10, masses=None, velocity="difference", gravity=(0.0, 0.0, 0.0),
                        state=None, animation="train", frame_start=0, frame_end=None, frame_jump=1, chunk_frames=None,
                        record_every=None, hyper=None, forces=None, floor=None, pins=None):
        """Extra: ``num_steps`` time steps of the reference's solver (Simulators.py ``step()``, :494-532) from every selected
        frame of the resident animation, on the device.  Every selected frame is an independent initial condition: positions
        x_f, velocity (x_f - x_{f-1}) / dt (``velocity`` "difference", f - 1 as in ``global_step``) or 0 ("zero").  A step is
        ``num_iterations`` local/global iterations from q_0 = s_t, then (:531-532) p_{t+1} = q and the next explicit state
        s_{t+1} = 2 q - p_t + dt^2 g -- the velocity (q - p_t) / dt carried into the next step.  Step 1 is
        ``solve_frames(start="explicit")`` bit for bit.  The state never leaves the device: the carry is one kernel on the
        iterate, the previous positions and the inertia term; the matrix, S^T V and A^-1 S^T V are formed once per call.

        ``kinds`` (one entry may be reduced; up to L after ``set_reduced_kinds(L)``, the banks and the union of the touched
        vertices set up once and carried through every step), ``dt``, ``num_iterations``, ``masses``, ``gravity``, ``animation``, the frame range,
        ``chunk_frames`` and ``hyper``: as ``solve_frames``, with its refusals.  ``state``: a pair ``(q, q_prev)`` of contiguous
        ``torch.float64`` device tensors (F', N, 3), the positions now and one step earlier: the roll-out continues from them
        (``velocity`` is then ignored and the animation only selects F'), and T1 steps continued by T2 equal T1 + T2 steps bit
        for bit.  ``record_every`` = r: also the positions after the steps r, 2 r, .. <= ``num_steps``.  ``pins``: the positional
        constraints of ``constraint_forces`` and ``solve_frames``; step t = 1, 2, .. of the roll-out from frame f reads row
        shift_start + f + t - 1 of the shift (the reference's step counter), so a continuation with ``state=`` passes
        ``shift_start`` raised by the steps already taken and then equals the longer roll-out bit for bit; a row beyond T_s is
        a ValueError before the device is touched.  ``forces``: None or a dict ``{force, vertices (None), start (0)}``, the
        reference's ``fext`` without gravity (Simulators.py:494-495): ``force`` (N, 3), constant, or (T_s, N, 3), one row per step;
        with ``vertices`` (P,), unique and in range, (P, 3) / (T_s, P, 3) and zero elsewhere.  Step t from frame f reads row
        ``start`` + f + t - 1, the pins' rule, and a continuation passes ``start`` raised by the steps taken.  The explicit state of
        a step becomes s + dt^2 force / mass (the table is formed on the host in f64, dense, at most 2^31 bytes on the device: a
        ValueError naming the size).  ``floor``: None or a dict ``{height, axis (1)}``, the reference's ``resolve_collision``
        (:497-498): coordinate ``axis`` of every vertex of the explicit state that lies below ``height`` is set onto it, before the
        iterations take their inertia term and first iterate from it.  Both are one pass with the carry; with
        both None nothing changes.  Unknown keys, wrong shapes, non-finite values, a missing row: ValueError before the device.

        Returns ``(q, q_prev, F')``: the positions after the last step and one step earlier (for ``num_steps`` = 1: x_f, or
        ``state[0]``), two ``torch.float64`` device tensors (F', N, 3) owned by the caller -- the pair ``state=`` takes.  With
        ``record_every`` a fourth value ``(records, steps)``: a caller-owned (R, F', N, 3) device tensor, each record written
        by the last iteration of its step straight into its slice, and the list of those step numbers; when the last step is
        recorded, ``q`` is the view ``records[-1]``.  Device memory held by the engine beside that of ``solve_frames``: one more
        tensor of the iterate's size, and the force table.  Out of scope: the self-collision passes, friction and repulsion,
        more reduced kinds than ``set_reduced_kinds`` allows (1 unless set), the history of step norms, several ranks."""
        who = "simulate_frames"
        self._hyper_check(who, hyper, kinds, False)
        ex, K = self._solve_args(who, dt, velocity, gravity, num_iterations, "explicit", masses)
        T, every = self._rollout_args(who, num_steps, record_every, state)
        frames = self._frames(animation, frame_start, frame_end, frame_jump)
        pins = self._pins(who, pins, frames, T)
        ext = self._external(who, forces, floor, ex, frames, T)
        plan, reds = self._solve_plan(who, kinds, chunk_frames)
        self._rollout_state(who, state, frames.n_sel)
        reds = self._chosen(reds, kinds)
        self._matrix(plan, ex.masses, ex.dt, pins)
        q, q_prev, records, steps = self._with_operators(
            reds, hyper, lambda: self._rollout_run(plan, reds, frames, ex, state, K, T, chunk_frames, every, hyper, pins, ext))
        return (q, q_prev, frames.n_sel) + (() if every is None else ((records, steps),))

    def reduced_rollout_errors(self, kind, basis, r_values, dt, num_steps, num_iterations=10, masses=None, velocity="difference",
                               gravity=(0.0, 0.0, 0.0), elements=None, wi=1.0, reduction="deim_pod", rest_positions=None,
                               sigma_min=1.0, sigma_max=1.0, animation="train", frame_start=0, frame_end=None, frame_jump=1,
                               record_every=1, hyper=None, forces=None, floor=None, pins=None):
        """Extra: how far the DEIM-reduced SIMULATION drifts from the full one along a trajectory -- ``reduced_solve_errors``
        carried through ``num_steps`` time steps of ``simulate_frames``.  For every r of ``r_values`` and every recorded step
        (``record_every`` = r0: the steps r0, 2 r0, .. <= ``num_steps``) the three metrics of ``(q_t, q~_{r,t})``: both roll-outs
        start at the same frames with the same velocity, the same A^-1 and the same masses, and from step 2 on each follows
        its own trajectory.  Arguments as ``reduced_solve_errors`` plus ``num_steps`` and ``record_every``; the start is the
        explicit state and there is no per-frame output.  The full roll-out runs once with its records, one reduced roll-out
        per r (S^T V and, with ``hyper``, A^-1 S^T V once, for the largest r); every record stays on the device and is compared
        there, slice by slice.

        Returns ``(fro, max, rel_x, rel_y, rel_z, steps)``: five (len(r_values), R) arrays and the list of the R recorded
        steps.  With ``num_steps=1, record_every=1`` the numbers are those of ``reduced_solve_errors``.  The sweep keeps its
        one kind whatever ``set_reduced_kinds`` allows: multi-kind sweeps are out of scope.  ``pins`` (as ``simulate_frames``)
        hold both roll-outs, unreduced: the hanging cloth, the clamped bar.  ``forces`` / ``floor`` (as ``simulate_frames``) act on
        both roll-outs alike: the drift under a load the basis was not trained on.  Out of scope: self-collisions, several ranks.
        (The sweep over the ranks of a position subspace is ``subspace_rollout_errors``.)"""
        who = "reduced_rollout_errors"
        self._hyper_check(who, hyper, [dict(basis=basis, num_components=0)], False)
        ex, K = self._solve_args(who, dt, velocity, gravity, num_iterations, "explicit", masses)
        T, every = self._rollout_args(who, num_steps, record_every, None)
        if every is None:
            raise ValueError("%s: record_every %r: a positive number of time steps" % (who, record_every))
        spec = dict(kind=kind, elements=elements, wi=wi, rest_positions=rest_positions, sigma_min=sigma_min, sigma_max=sigma_max)
        frames = self._frames(animation, frame_start, frame_end, frame_jump)
        pins = self._pins(who, pins, frames, T)
        ext = self._external(who, forces, floor, ex, frames, T)
        terms, (red,) = self._solve_plan(who, [dict(spec, basis=basis, num_components=0, reduction=reduction)], None)
        r_values = [int(r) for r in r_values]
        ops = [red.operator(r) for r in r_values]
        steps = list(range(every, T + 1, every))
        out = np.zeros((5, len(ops), len(steps)))
        if not ops:
            return tuple(out) + (steps,)
        run = lambda rd: self._rollout_run(terms, () if rd is None else (rd,), frames, ex, None, K, T, None, every, None if rd is None else hyper,
                                           pins, ext, True)[2]
        self._matrix(terms, ex.masses, ex.dt, pins)
        if ext is not None:
            self._ext_set(ext)
        full = run(None)
        self._engine.rforce_operator(terms[0].St, ops[int(np.argmax(r_values))].V)
        if hyper is not None:
            self._engine.hyper_operator()
        for i, op in enumerate(ops):
            rec = run(red._replace(op=op))
            for j in range(len(steps)):
                out[:, i, j] = [m[0] for m in self._diff_metrics(full[j], [rec[j]], frames.n_sel, False)]
        return tuple(out) + (steps,)

    # ------------------------------------------------------------------ roll-outs whose state lives in z
    def _subspace_held(self, who):
        """r of the subspace on the device, or the ValueError of a call that needs one."""
        self._one_rank(who)
        if self._subspace_solver() is None or getattr(self, "global_solve_subspace", None) is None or getattr(self, "global_matrix", None) is None:
            raise ValueError("%s: no position subspace on the device: set_global_solver('subspace', basis=...) and global_solve_setup "
                             "(or a solve) first" % who)
        return int(self.global_solve_subspace)

    def _z_tensor(self, who, name, t, rows, n_sel=None):
        """A caller's ``torch.float64`` device tensor (F', rows, 3), contiguous, on the snapshots' device; F' = ``n_sel`` if given."""
        import torch
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or not t.is_cuda:
            raise ValueError("%s: %s must be a torch.float64 device tensor" % (who, name))
        if t.device.index != self._engine.device_id:
            raise ValueError("%s: %s lives on %s, the snapshots on device %d" % (who, name, t.device, self._engine.device_id))
        if t.dim() != 3 or t.shape[0] < 1 or tuple(t.shape[1:]) != (rows, 3) or (n_sel is not None and t.shape[0] != n_sel) or not t.is_contiguous():
            raise ValueError("%s: %s of shape %s: a contiguous (%s, %d, 3) expected" % (who, name, tuple(t.shape), "F'" if n_sel is None else n_sel, rows))
        return t

    def subspace_coordinates(self, positions="train", frame_start=0, frame_end=None, frame_jump=1):
        """Extra: the coordinates z = U^T (x - o) of positions in the subspace the device holds (``set_global_solver("subspace")``
        and a matrix set-up), per coordinate the Euclidean projection onto the orthonormalised basis.  ``positions``: "train" or
        "test" with the frame range of ``constraint_forces``, or a contiguous ``torch.float64`` device tensor (F', N, 3) in world
        space.  Returns a caller-owned ``torch.float64`` device tensor (F', r, 3).  One pass over N; the sum over the vertices is
        never split.  One rank only."""
        import torch
        who = "subspace_coordinates"
        r = self._subspace_held(who)
        eng = self._engine
        if isinstance(positions, str):
            if positions not in ("train", "test"):
                raise ValueError("%s: positions must be 'train', 'test' or a torch.float64 device tensor (F', %d, 3), not %r" % (who, self.nVerts, positions))
            frames = self._frames(positions, frame_start, frame_end, frame_jump)
            frames.upload(self)
            out = self._alloc(frames, r)
            eng.gsub_coordinates(*frames.args(self), out.data_ptr())
            return out
        x = self._z_tensor(who, "positions", positions, self.nVerts)
        torch.cuda.current_stream(x.device).synchronize()           # whatever produced the tensor is done before the engine reads it
        out = torch.empty((x.shape[0], r, 3), dtype=torch.float64, device=x.device)
        eng.gsub_coordinates(0, 0, 1, 1, None, False, 1.0, out.data_ptr(), x.data_ptr(), x.shape[0])
        return out

    def subspace_expand(self, z):
        """Extra: q = o + U z for a contiguous ``torch.float64`` device tensor ``z`` (F', r, 3) of coordinates in the subspace the
        device holds: a caller-owned device tensor (F', N, 3) in world space.  One rank only."""
        import torch
        who = "subspace_expand"
        r = self._subspace_held(who)
        z = self._z_tensor(who, "z", z, r)
        torch.cuda.current_stream(z.device).synchronize()
        out = torch.empty((z.shape[0], self.nVerts, 3), dtype=torch.float64, device=z.device)
        self._engine.gsub_expand(z.data_ptr(), z.shape[0], out.data_ptr())
        return out

    def simulate_subspace(self, kinds, dt, num_steps, num_iterations=10, masses=None, velocity="difference", gravity=(0.0, 0.0, 0.0),
                          state=None, animation="train", frame_start=0, frame_end=None, frame_jump=1, chunk_frames=None,
                          record_every=None, pins=None, forces=None, floor=None):
        """Extra: ``simulate_frames(hyper="touched")`` under ``set_global_solver("subspace")`` with the STATE kept in the subspace
        coordinates z of q = o + U z -- the reference's fully reduced simulator (Simulators.py:144-155, :195, :239, where it raises
        "not yet implemented").  Per coordinate, with At = U^T A U: a step is y = 2 z_t - z_{t-1}, c_z = kappa + T y + E target,
        then ``num_iterations`` times z <- c_z + sum_k Gz_k coef_k(q) with q = o + U z formed at the touched vertices only.
        T = At^-1 U^T (M / dt^2) U, kappa, E (the pins) and Gz_k = At^-1 U^T S_k^T V_k are formed once per call; a time step
        reads and writes nothing of size N.  For frames inside o + span(U) this is ``simulate_frames(hyper=)``
        under the subspace up to rounding; frames outside start from their Euclidean projection z_0 = U^T (x_f - o).

        Arguments as ``simulate_frames`` without ``hyper``; EVERY kind must be reduced (up to ``set_reduced_kinds`` of them).
        ``state``: a pair ``(z, z_prev)`` of contiguous ``torch.float64`` device tensors (F', r, 3) continues a roll-out
        (``velocity`` is then ignored, the animation only selects F'; pins take ``shift_start`` raised by the steps already taken):
        T1 steps continued by T2 equal T1 + T2 steps bit for bit.  Returns ``(z, z_prev, F')``: caller-owned device tensors
        (F', r, 3); with ``record_every`` also ``(records (R, F', r, 3), steps)``.  ``subspace_expand`` gives the positions.
        ValueError before the device is touched: no subspace selected, a plain kind, a bad ``state``, a row of the pins' shift
        beyond T_s.  ``forces``: the dict of ``simulate_frames`` (a continuation passes ``start`` raised by the steps taken): with
        Phi = At^-1 U^T applied to the table's rows, formed once per call, c_z gains Phi[:, row] and the touched rows of a step's first
        iterate gain fa[row]; at most 65 535 rows.  ``floor`` is refused (ValueError): a clamp on vertex coordinates
        has no form in z without the O(N) pass this roll-out exists to avoid -- ``simulate_frames`` under
        ``set_global_solver("subspace")`` takes it.  Out of scope: plain kinds, the history of step norms, several ranks."""
        import torch
        who = "simulate_subspace"
        self._one_rank(who)
        sub = self._subspace_solver()
        if sub is None:
            raise ValueError("%s: the state lives in the coordinates of a position subspace: set_global_solver('subspace', basis=...) first" % who)
        if floor is not None:
            raise ValueError("%s: floor=: a clamp on vertex coordinates has no form in the subspace coordinates z without the O(N) pass "
                             "over the vertices that this roll-out exists to avoid; simulate_frames under set_global_solver('subspace') takes "
                             "floor= (and forces=)" % who)
        r = int(sub[0].shape[1])
        limit = getattr(self, "_reduced_limit", 1)
        if not (isinstance(kinds, (list, tuple)) and len(kinds) >= 1 and all(
                isinstance(k, dict) and "basis" in k and "num_components" in k for k in kinds)):
            raise ValueError("%s: every kind must be reduced ('basis' and 'num_components'): up to %d of them under set_reduced_kinds(%d), "
                             "none left plain" % (who, limit, limit))
        ex, K = self._solve_args(who, dt, velocity, gravity, num_iterations, "explicit", masses)
        T, every = self._rollout_args(who, num_steps, record_every, None)
        frames = self._frames(animation, frame_start, frame_end, frame_jump)
        pins = self._pins(who, pins, frames, T)
        ext = self._external(who, forces, None, ex, frames, T)
        if ext is not None and ext.forces.table.ndim == 2 and ext.forces.table.shape[0] > 65535:
            raise ValueError("%s: forces: %d rows of force, at most 65535 in a roll-out in z (continue with state= and start raised)"
                             % (who, ext.forces.table.shape[0]))
        plan, reds = self._solve_plan(who, kinds, chunk_frames)
        if state is not None:
            if not isinstance(state, (list, tuple)) or len(state) != 2:
                raise ValueError("%s: state must be a pair (z, z_prev) of torch.float64 device tensors" % who)
            state = tuple(self._z_tensor(who, "state", t, r, frames.n_sel) for t in state)
        reds = self._chosen(reds, kinds)
        self._matrix(plan, ex.masses, ex.dt, pins)
        eng, multi = self._engine, len(reds) > 1
        try:
            for b, rd in enumerate(reds):
                if multi:
                    eng.rforce_bank(b)
                eng.rforce_operator(rd.St, rd.op.V)
                eng.zroll_operator()
            if state is not None:
                torch.cuda.current_stream(state[0].device).synchronize()
            frames.upload(self)
            if pins is not None:
                self._pins_set(pins)
            if ext is not None:
                self._ext_set(ext)
            touched, sampled = self._sampled(reds, "touched")
            eng.zroll_begin(*frames.args(self), ex.diag, ex.mode, ex.acc, touched,
                            None if state is None else state[0].data_ptr(), None if state is None else state[1].data_ptr())
            if ext is not None:
                eng.zroll_forces(ext.forces.start)
            if pins is not None:
                eng.zroll_pins(pins.start)
            for b, rd in enumerate(reds):
                if multi:
                    eng.rforce_bank(b)
                eng.cproj_setup(sampled[rd.index])
                eng.rforce_solver(rd.op.H, rd.op.local_rows)
                eng.zroll_slot(plan[rd.index].sigma_min, plan[rd.index].sigma_max)
            steps = [] if every is None else list(range(every, T + 1, every))
            dev = "cuda:%d" % eng.device_id
            records = None if every is None else torch.empty((len(steps), frames.n_sel, r, 3), dtype=torch.float64, device=dev)
            eng.zroll_steps(T, K, 0 if chunk_frames is None else int(chunk_frames), 0 if every is None else every,
                            None if records is None or not steps else records.data_ptr())
            z, z_prev = self._alloc(frames, r), self._alloc(frames, r)
            eng.zroll_state(z.data_ptr(), z_prev.data_ptr())
        finally:
            if multi:
                eng.rforce_bank(0)
        self._leave(plan, pins)
        return (z, z_prev, frames.n_sel) + (() if every is None else ((records, steps),))

    # ------------------------------------------------------------------ the position subspace judged along roll-outs
    def subspace_distance(self, positions, z, per_frame=False):
        """Extra: the reference's three metrics (constraintsComponents.py:524-556) of ``(positions, o + U z)`` for the subspace
        the device holds -- ``fro, max, rel_x, rel_y, rel_z`` as scalars, with the arithmetic of the ``reduced_*_errors`` sweeps --
        and, with ``per_frame``, a sixth value: the (F',) array |x_f - q~_f| / |x_f|.  ``positions``: a contiguous
        ``torch.float64`` device tensor (F', N, 3) in world space; ``z``: one of (F', r, 3).  o + U z is formed tile by tile with the
        bits of ``subspace_expand`` and compared in registers (csrc/asb_zroll.hip): ``positions`` is read once and
        no (F', N, 3) tensor is written.  Both tensors are checked, F' included, before the device is touched.  One rank only."""
        import torch
        who = "subspace_distance"
        r = self._subspace_held(who)
        x = self._z_tensor(who, "positions", positions, self.nVerts)
        z = self._z_tensor(who, "z", z, r, int(x.shape[0]))
        torch.cuda.current_stream(z.device).synchronize()           # whatever produced the tensors is done before the engine reads them
        out = self._metrics(*self._engine.gsub_expand_diff(x.data_ptr(), z.data_ptr(), int(x.shape[0]), per_frame))
        return out if per_frame else out[:5]

    def subspace_rollout_errors(self, kinds, basis, r_values, dt, num_steps, num_iterations=10, masses=None, velocity="difference",
                                gravity=(0.0, 0.0, 0.0), animation="train", frame_start=0, frame_end=None, frame_jump=1, chunk_frames=None,
                                record_every=1, pins=None, forces=None, origin=None, baseline="reduced"):
        """Extra: how far a roll-out in a POSITION subspace drifts from one without it -- ``subspace_solve_errors`` carried through
        ``num_steps`` time steps.  For every r of ``r_values`` and every recorded step (``record_every`` = r0: the steps r0, 2 r0, ..
        <= ``num_steps``) the three metrics of ``(q_t, o + U_r z_t)``: q_t from ONE baseline roll-out with records under the solver
        selected now ("inverse" or "slab"; under "subspace" a ValueError), z_t from ``simulate_subspace`` under
        ``set_global_solver("subspace", basis=basis, num_components=r, origin=origin)`` with the same arguments.  ``baseline``
        "reduced": ``simulate_frames(kinds, .., hyper="touched")``, so the drift is the position subspace's alone; "full": the same
        call with the reduction keys of every kind taken off and no ``hyper``, the drift of the whole reduced simulator against the
        unreduced one.  Arguments as ``simulate_subspace`` (EVERY kind reduced; no ``state``, and no ``floor``, which it refuses).

        A roll-out in z starts from the Euclidean projection z_0 = U^T (x_f - o) of the frames (z_-1 likewise), the baseline from the
        frames themselves: the errors of every step INCLUDE the projection error of the start, carried through the dynamics.

        Per r: one subspace set-up (kept if the device holds that very one), one roll-out in z with its records, and per recorded
        step one fused expansion + comparison on the slices (``full[j]``, ``z[j]``) -- no expansion is stored and no (F', N, 3)
        tensor is made per r.  Memory held by the call: the baseline's R records, 24 R F' N bytes, and the R records
        of one roll-out in z, 24 R F' r bytes.  Checked before the device is touched: every r (rank included), every kind reduced,
        ``record_every``, ``baseline``, the rows of ``pins`` and ``forces`` for ``num_steps``, at most 65 535 rows of force.

        Returns ``(fro, max, rel_x, rel_y, rel_z, steps)``: five (len(r_values), R) arrays and the list of the R recorded steps,
        the shape of ``reduced_rollout_errors``; an empty ``r_values`` gives (0, R) arrays and touches no engine.  The solver
        selected for this object is the same afterwards, also after an exception.  One rank only."""
        who = "subspace_rollout_errors"
        self._one_rank(who)
        if self._subspace_solver() is not None:
            raise ValueError("%s: the full solve runs under 'inverse' or 'slab': set_global_solver('subspace') is in force" % who)
        if baseline not in ("reduced", "full"):
            raise ValueError("%s: baseline must be 'reduced' or 'full', not %r" % (who, baseline))
        subs = [self._subspace_args(who, basis, r, origin) for r in r_values]     # (r unchanged: 2.5 and True are refused)
        limit = getattr(self, "_reduced_limit", 1)
        keys = ("basis", "num_components", "reduction")
        if not (isinstance(kinds, (list, tuple)) and len(kinds) >= 1 and all(
                isinstance(k, dict) and "basis" in k and "num_components" in k for k in kinds)):
            raise ValueError("%s: every kind must be reduced ('basis' and 'num_components'): up to %d of them under set_reduced_kinds(%d), "
                             "none left plain" % (who, limit, limit))
        if baseline == "reduced":
            self._hyper_check(who, "touched", kinds, False)
        ex, K = self._solve_args(who, dt, velocity, gravity, num_iterations, "explicit", masses)
        T, every = self._rollout_args(who, num_steps, record_every, None)
        if every is None:
            raise ValueError("%s: record_every %r: a positive number of time steps" % (who, record_every))
        frames = self._frames(animation, frame_start, frame_end, frame_jump)
        self._pins(who, pins, frames, T)
        ext = self._external(who, forces, None, ex, frames, T)
        if ext is not None and ext.forces.table.ndim == 2 and ext.forces.table.shape[0] > 65535:
            raise ValueError("%s: forces: %d rows of force, at most 65535 in a roll-out in z (continue with state= and start raised)"
                             % (who, ext.forces.table.shape[0]))
        self._solve_plan(who, kinds, chunk_frames)
        steps = list(range(every, T + 1, every))
        out = np.zeros((5, len(subs), len(steps)))
        if not subs:
            return tuple(out) + (steps,)
        args = dict(masses=masses, velocity=velocity, gravity=gravity, animation=animation, frame_start=frame_start, frame_end=frame_end,
                    frame_jump=frame_jump, chunk_frames=chunk_frames, record_every=every, pins=pins, forces=forces)
        if baseline == "reduced":
            full = self.simulate_frames(kinds, dt, T, K, hyper="touched", **args)[3][0]
        else:
            full = self.simulate_frames([{k: v for k, v in spec.items() if k not in keys} for spec in kinds], dt, T, K, hyper=None, **args)[3][0]
        selected = (self._global_solver if hasattr(self, "_global_solver") else None, getattr(self, "_global_subspace", None))
        try:
            for i, sub in enumerate(subs):
                self._global_solver, self._global_subspace = ("subspace", None), sub
                zrec = self.simulate_subspace(kinds, dt, T, K, **args)[3][0]
                for j in range(len(steps)):
                    out[:, i, j] = self._metrics(*self._engine.gsub_expand_diff(full[j].data_ptr(), zrec[j].data_ptr(), frames.n_sel))[:5]
        finally:
            if selected[0] is None:
                del self._global_solver
            else:
                self._global_solver = selected[0]
            self._global_subspace = selected[1]
        return tuple(out) + (steps,)
