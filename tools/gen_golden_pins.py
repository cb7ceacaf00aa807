"""Writes tests/golden/pins_<name>.npz for the fixtures of tests/pins_cases.py (CPU only; never imported by a test).

    python tools/gen_golden_pins.py

What the UNMODIFIED reference's own code produces with positional constraints: its ``PositionalConstraint`` objects
(Constraint_projections.py:77-113; ``motion_type='fixed'``, or ``'user_defined'`` with one ``frame_shift`` (T_s, 3) per pin) beside
the element constraints of tools/gen_golden_rollout.py, all of them handed to its ``prepare_global_matrix`` (Simulators.py:117-145,
through ``reference_solver`` of tools/gen_golden_gstep.py), whose factorisation does every solve.  The loop of ``step()`` is
written out here (:494-532), because its positional term calls ``get_pi(q, frame)`` with the step counter ``self.frame`` (:407),
which ``reference_loop`` of tools/gen_golden_pdsolve.py does not pass:

    a = fext / mass;  explicit = positions + dt velocities + dt^2 a                     (:494-495; fext = mass g)
    K times:  b = S_pos^T p_pos(frame) + sum of the kinds' S^T p(q) + M / dt^2 explicit;  q = cholesky(b)     (:506-526)
    velocities = (q - positions) / dt;  positions = q;  frame += 1                      (:531-534)

The counter starts at the start frame f (the reference's step from the state of frame f is its step number f).

Per fixture: ``g_<mode>`` (44, N, 3), one iteration from q = x_f (``global_step``); ``q_<mode>_<K>_<T>``, the positions after T
steps of K iterations from the explicit state (T = 1: ``solve_frames``), for the start frames range(0, 130, 3), both explicit
states, gravity ``pins_cases.G``, K in {1, 3, 10}; ``amp_<mode>_<K>_<T>``, the amplification tests/pins_cases.py measures ON ITS HOST
MODEL; ``row`` / ``col`` / ``val`` / ``shape``, the N x N block A_N of the matrix the reference's triplets sum to, pins included.
A (mode, K, T) whose amplification exceeds ``pdsolve_cases.AMP_CAP`` = 1e3 is dropped with a printed line, and the kept
ones are asserted to stay under it; ``steps`` lists the T that every mode and K kept."""
import os
import sys

import numpy as np
from scipy import sparse

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
from gen_golden_cproj import save      # noqa: E402
from gen_golden_gstep import DT, WI, load, masses_of, reference_solver, triplet_matrix      # noqa: E402
from gen_golden_pdsolve import P_ROWS      # noqa: E402
from gen_reduced_forces_golden import import_reference_simulator      # noqa: E402
import pdsolve_cases as pc      # noqa: E402
import pins_cases as pins      # noqa: E402
import rollout_cases as rc      # noqa: E402


def element_groups(CP, base):
    """Per kind of the element set: the reference's constraints, their rows per element and their assembly matrix."""
    out = []
    for kind in pc.parts_of(base):
        g = load("cproj_" + kind)
        rest, el, sig = g["rest"], g["elements"], g["sigma"]
        if kind == "edge_spring":
            cs = [CP.EdgeSpringConstraint(e.tolist(), WI, rest) for e in el]
        elif kind == "tris_strain":
            cs = [CP.TriStrainConstraint(t.tolist(), WI, rest, *sig) for t in el]
        elif kind == "tets_strain":
            cs = [CP.TetStrainConstraint(t.tolist(), WI, rest, *sig) for t in el]
        else:
            cs = [CP.TetDeformationGradientConstraint(t.tolist(), WI, rest) for t in el]
        out.append((cs, P_ROWS[kind], sparse.hstack([c._selection_matrix for c in cs]).tocsr()))
    return out


def positional(CP, spec, rest):
    """The reference's positional constraints of a ``pins=`` dict and their assembly matrix (``add_positional_constraint``,
    :1164-1176: one constraint per vertex)."""
    shift = spec.get("shift")
    cs = []
    for i, (v, w) in enumerate(zip(spec["vertices"], spec["wi"])):
        if shift is None:
            cs.append(CP.PositionalConstraint([int(v)], float(w), rest))
        else:
            cs.append(CP.PositionalConstraint([int(v)], float(w), rest, motion_type="user_defined", frame_shift=shift[:, i]))
    return cs, sparse.hstack([sparse.csr_matrix(c._selection_matrix) for c in cs]).tocsr()


def reference_iterations(solve, groups, pos, mass, dt, explicit, q, frame, K):
    """Simulators.py:500-526 for one frame: K iterations from ``q`` with the explicit state ``explicit`` and the step counter
    ``frame``."""
    N = explicit.shape[0]
    dt2_inv = 1.0 / (dt * dt)
    sn = explicit.flatten()
    masses = np.zeros(3 * N)
    for i in range(N):
        masses[3 * i:3 * i + 3] = dt2_inv * mass[i] * sn[3 * i:3 * i + 3]
    q = q.flatten()
    pcs, pSt = pos
    for _ in range(K):
        b = np.zeros((N, 3))
        stacked = np.zeros((pSt.shape[1], 3))                      # :401-412
        for i, c in enumerate(pcs):
            stacked[i, :] = c.get_pi(q, frame)
        result = [pSt @ stacked]
        for cs, p, St in groups:
            stacked = np.zeros((St.shape[1], 3))
            for i, c in enumerate(cs):
                stacked[p * i:p * i + p, :] = c.get_pi(q)
            result.append(St @ stacked)
        b += sum(result)                                           # :520
        b += masses.reshape(N, 3)                                  # :524
        q = solve(b.flatten())
    return q.reshape(N, 3)


def reference_rollout(solve, groups, pos, mass, dt, g, x, x_prev, mode, f, K, steps):
    """{T: q (N, 3)} for the start frame ``f``: ``step()`` written out, the counter starting at f."""
    positions = x.copy()
    velocities = np.zeros_like(x) if mode == "zero" else (x - x_prev) / dt
    fext = mass[:, None] * np.asarray(g)[None, :]
    out, frame = {}, f
    for t in range(1, max(steps) + 1):
        a = fext / mass[:, None]                                   # :494
        explicit = positions + dt * velocities + dt * dt * a       # :495
        q_next = reference_iterations(solve, groups, pos, mass, dt, explicit, explicit, frame, K)
        velocities = (q_next - positions) * (1.0 / dt)             # :531
        positions = q_next                                         # :532
        frame += 1                                                 # :534
        if t in steps:
            out[t] = q_next.copy()
    return out


def record(CP, Simulators, name):
    fx = pins.FIXTURES[name]
    g = load("cproj_" + pc.parts_of(fx["base"])[-1])
    rest, frames = g["rest"], g["frames"]
    N = frames.shape[1]
    mass = masses_of(N)
    spec = pins.pins_of(name, rest)
    groups = element_groups(CP, fx["base"])
    pos = positional(CP, spec, rest)
    constraints = [c for gr in groups for c in gr[0]] + pos[0]
    solve = reference_solver(Simulators, constraints, rest, mass, DT)
    D = triplet_matrix(constraints, mass, DT).toarray()            # the matrix those triplets sum to: kron(A_N, I_3)
    A_N = sparse.coo_matrix(D[0::3, 0::3])
    assert np.array_equal(np.kron(D[0::3, 0::3], np.eye(3)), D)
    case = pins.host_case(name, load=load)
    sel, steps = rc.START_FRAMES, pins.steps_of(name)
    acc = DT * DT * np.array(pins.G)
    arrays, kept = {}, set(steps)
    for mode in pc.MODES:
        s, x = rc.start_state(frames, sel, mode, acc)
        prev = frames[[max(f - 1, 0) for f in sel]]
        fext_a = (mass[:, None] * np.array(pins.G)[None, :]) / mass[:, None]
        gs = np.empty_like(x)
        for i, f in enumerate(sel):                                # one iteration from the frame: global_step
            explicit = x[i] + DT * (np.zeros_like(x[i]) if mode == "zero" else (x[i] - prev[i]) / DT) + DT * DT * fext_a
            gs[i] = reference_iterations(solve, groups, pos, mass, DT, explicit, x[i], f, 1)
        arrays["g_%s" % mode] = gs
        host_g = pins.iterate(case, s, x, 1, sel)
        print("%-20s %-10s global step: |host model - reference| %.3g" % (name, mode, np.abs(host_g - gs).max()), flush=True)
        for K in pc.KS:
            q = {T: np.empty_like(x) for T in steps}
            for i, f in enumerate(sel):
                got = reference_rollout(solve, groups, pos, mass, DT, pins.G, x[i], prev[i], mode, f, K, steps)
                for T in steps:
                    q[T][i] = got[T]
            amp = pins.measure_amp(case, mode, K, max(steps), sel, acc)
            host = pins.rollout(case, K, max(steps), s, x, sel, acc)
            for T in steps:
                line = "%-20s %-10s K = %2d T = %d: amp %.3g, |host model - reference| %.3g" % (
                    name, mode, K, T, amp[T - 1], np.abs(host[T - 1] - q[T]).max())
                if amp[T - 1] > pc.AMP_CAP:
                    kept.discard(T)
                    print(line + "  -- DROPPED: over the cap %g" % pc.AMP_CAP, flush=True)
                    continue
                print(line, flush=True)
                arrays["q_%s_%d_%d" % (mode, K, T)] = q[T]
                arrays["amp_%s_%d_%d" % (mode, K, T)] = np.float64(amp[T - 1])
    kept = sorted(kept)
    arrays = {k: v for k, v in arrays.items() if k.startswith("g_") or int(k.rsplit("_", 1)[1]) in kept}
    for k, v in arrays.items():
        if k.startswith("amp_"):
            assert float(v) <= pc.AMP_CAP, (name, k, float(v))
    print("%s keeps the steps %s" % (name, kept))
    extra = {} if "shift" not in spec else {"shift": spec["shift"]}
    save("pins_" + name, dt=np.float64(DT), wi=np.float64(WI), Ks=np.array(pc.KS, dtype=np.int64), steps=np.array(kept, dtype=np.int64),
         start_frames=np.array(sel, dtype=np.int64), gravity=np.array(pins.G), vertices=spec["vertices"], pin_wi=spec["wi"],
         positions=spec["positions"], row=A_N.row.astype(np.int64), col=A_N.col.astype(np.int64), val=A_N.data.astype(np.float64),
         shape=np.array(A_N.shape, dtype=np.int64), **extra, **arrays)


def main():
    CP, Simulators = import_reference_simulator()
    for name in sorted(pins.FIXTURES):
        record(CP, Simulators, name)


if __name__ == "__main__":
    main()
