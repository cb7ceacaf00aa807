"""Writes tests/golden/forces_<name>.npz for the fixtures of tests/forces_cases.py (CPU only; never imported by a test).

    python tools/gen_golden_forces.py

What the UNMODIFIED reference's own code produces with external forces and its floor.  ``step(fext, num_iterations)`` is written
out here around the reference's pieces, because its self-collision passes (:529-530) need a library this project does not use and
are out of scope:

    fext = mass g + force[row]                                                         (usr_interface.py:163)
    a = fext / mass;  explicit = positions + dt velocities + dt^2 a                    (:494-495)
    DeformableMesh.resolve_collision(v, explicit, corrections) for every vertex v      (:497-498; called unbound on a namespace
                                                                                        that carries foolr_collision = True and floor_height)
    K times:  b = sum of the kinds' S^T p(q) + M / dt^2 explicit;  q = cholesky(b)     (:506-526, ``reference_iterations`` of gen_golden_pins.py)
    velocities = (q - positions) / dt;  positions = q;  row += 1                       (:531-534)

The row starts at the start frame f, as the pins' step counter does.

Per fixture: ``q_<mode>_<K>_<T>`` (44, N, 3), the positions after T steps of K iterations from the explicit state (T = 1:
``solve_frames``), for the start frames range(0, 130, 3), both explicit states, gravity ``forces_cases.G``, K in {1, 3, 10};
``amp_<mode>_<K>_<T>``, the amplification tests/forces_cases.py measures ON ITS HOST MODEL with the table and the floor in the loop;
``share_<mode>_<K>`` (kept steps,), the share of (frame, vertex) pairs the REFERENCE clamped at each kept step; ``force`` (T_S, N, 3),
``floor`` (the height; absent without one), ``gravity``, ``start_frames``, ``steps``.  A (mode, K, T) whose amplification exceeds
``pdsolve_cases.AMP_CAP`` = 1e3 is dropped with a printed line; the kept ones are asserted to stay under it, and every kept floor
case to clamp between 5 % and 95 % at every step up to its largest kept T."""
import os
import sys
import types

import numpy as np
from scipy import sparse

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
from gen_golden_cproj import save      # noqa: E402
from gen_golden_gstep import DT, load, masses_of, reference_solver      # noqa: E402
from gen_golden_pins import element_groups, reference_iterations      # noqa: E402
from gen_reduced_forces_golden import import_reference_simulator      # noqa: E402
import forces_cases as fc      # noqa: E402
import pdsolve_cases as pc      # noqa: E402
import rollout_cases as rc      # noqa: E402


def reference_rollout(CP, solve, groups, mass, dt, g, force, floor, x, x_prev, mode, f, K, T):
    """([q_1, .., q_T], [clamped vertices of step 1, .., T]) for the start frame ``f``: ``step()`` written out."""
    N = x.shape[0]
    positions = x.copy()
    velocities = np.zeros_like(x) if mode == "zero" else (x - x_prev) / dt
    none = ([], sparse.csr_matrix((N, 0)))
    model = types.SimpleNamespace(foolr_collision=floor is not None, floor_height=floor, m_collisionCorrection=False)
    out, hits, row = [], [], f
    for t in range(T):
        fext = mass[:, None] * np.asarray(g)[None, :] + force[row]  # usr_interface.py:163
        a = fext / mass[:, None]                                   # :494
        explicit = positions + dt * velocities + dt * dt * a       # :495
        before = explicit.copy()
        corrections = np.zeros_like(explicit)
        for v in range(N):                                         # :497-498
            CP.DeformableMesh.resolve_collision(model, v, explicit, corrections)
        hits.append(int((explicit[:, 1] != before[:, 1]).sum()))
        q_next = reference_iterations(solve, groups, none, mass, dt, explicit, explicit, row, K)
        velocities = (q_next - positions) * (1.0 / dt)             # :531
        positions = q_next                                         # :532
        row += 1                                                   # :534
        out.append(q_next.copy())
    return out, hits


def record(CP, Simulators, name):
    g = load("cproj_" + name)
    rest, frames = g["rest"], g["frames"]
    N = frames.shape[1]
    mass = masses_of(N)
    groups = element_groups(CP, name)
    solve = reference_solver(Simulators, [c for gr in groups for c in gr[0]], rest, mass, DT)
    case = pc.host_case(name, load)
    assert np.array_equal(case["masses"], mass) and case["dt"] == DT
    sel, steps = rc.START_FRAMES, fc.steps_of(name)
    T = max(steps)
    acc = DT * DT * np.array(fc.G)
    force = fc.force_of(N)
    fa = fc.fa_of(force, mass, DT)
    height = fc.floor_of(name, frames, acc)
    floor = None if height is None else (height, 1)
    arrays, kept = {}, set(steps)
    for mode in pc.MODES:
        s, x = rc.start_state(frames, sel, mode, acc)
        prev = frames[[max(f - 1, 0) for f in sel]]
        for K in pc.KS:
            q = np.empty((T,) + x.shape)
            hits = np.zeros(T)
            for i, f in enumerate(sel):
                got, h = reference_rollout(CP, solve, groups, mass, DT, fc.G, force, height, x[i], prev[i], mode, f, K, T)
                q[:, i] = got
                hits += h
            share = hits / (len(sel) * N)
            amp = fc.measure_amp(case, mode, K, T, sel, acc, fa, floor)
            host_share = []
            host = fc.rollout(case, K, T, s, x, sel, acc, fa, floor, shares=host_share)
            arrays["share_%s_%d" % (mode, K)] = share
            for t in steps:
                line = "%-26s %-10s K = %2d T = %d: amp %.3g, clamped share %.3f (host model %.3f), |host model - reference| %.3g" % (
                    name, mode, K, t, amp[t - 1], share[t - 1], host_share[t - 1], np.abs(host[t - 1] - q[t - 1]).max())
                if amp[t - 1] > pc.AMP_CAP:
                    kept.discard(t)
                    print(line + "  -- DROPPED: over the cap %g" % pc.AMP_CAP, flush=True)
                    continue
                print(line, flush=True)
                arrays["q_%s_%d_%d" % (mode, K, t)] = q[t - 1]
                arrays["amp_%s_%d_%d" % (mode, K, t)] = np.float64(amp[t - 1])
    kept = sorted(kept)
    assert kept and kept[0] == 1, (name, kept)
    out = {}
    for k, v in arrays.items():
        if k.startswith("share_"):
            out[k] = v[:max(kept)]
            if floor is not None:
                fc.check_shares(out[k])
        elif int(k.rsplit("_", 1)[1]) in kept:
            out[k] = v
            if k.startswith("amp_"):
                assert float(v) <= pc.AMP_CAP, (name, k, float(v))
    print("%s keeps the steps %s" % (name, kept))
    extra = {} if height is None else {"floor": np.float64(height)}
    save("forces_" + name, dt=np.float64(DT), Ks=np.array(pc.KS, dtype=np.int64), steps=np.array(kept, dtype=np.int64),
         start_frames=np.array(sel, dtype=np.int64), gravity=np.array(fc.G), force=force, **extra, **out)


def main():
    CP, Simulators = import_reference_simulator()
    for name in sorted(fc.FIXTURES):
        record(CP, Simulators, name)


if __name__ == "__main__":
    main()
