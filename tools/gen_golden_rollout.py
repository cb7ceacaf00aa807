"""Writes tests/golden/rollout_<name>.npz for the five pdsolve fixtures and rollout_reduced_<fixture>.npz (CPU only; never
imported by a test).

    python tools/gen_golden_rollout.py [--reduced-only]

rollout_<name>: what the UNMODIFIED reference's own code produces over several time steps: per step ``reference_loop`` of
tools/gen_golden_pdsolve.py (Simulators.py:500-526: the constraints, the factorisation and the b of that tool), and between
steps the last two lines of ``step()`` (:531-532) with the explicit state of the next step (:495),

    velocities = (q_next - positions) / dt;  positions = q_next;  explicit = positions + dt velocities

(no external acceleration).  Start frames range(0, 130, 3) of the cproj fixture, both explicit states of pdsolve (``zero``:
velocity 0, ``difference``: (x_f - x_{f-1}) / dt), K in {1, 3, 10}: ``q_<mode>_<K>_<T>`` (44, N, 3) is the position after T
steps, T in ``rollout_cases.STEPS[name]``, and ``amp_<mode>_<K>_<T>`` the amplification tests/rollout_cases.py measures ON ITS
HOST MODEL (perturbed states and first iterates; its docstring), which the tests' bound uses and which must stay <= 1e3.

rollout_reduced_<fixture>: ``amp_<m>_<mode>_<K>_<T>`` of the host model with the kind reduced to m components (smallest and
largest m of reduced_forces_<fixture>.npz) and ``steps``: the longest prefix of (2, 5, 8) at which every one of them is
<= 1e3 (the reduced roll-out has no reference run; the tests compare the device with the host route)."""
import os
import sys

import numpy as np
from scipy import sparse

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
from gen_golden_cproj import save      # noqa: E402
from gen_golden_gstep import DT, WI, load, masses_of, reference_solver      # noqa: E402
from gen_golden_pdsolve import P_ROWS, reference_loop      # noqa: E402
from gen_reduced_forces_golden import import_reference_simulator      # noqa: E402
import pdsolve_cases as pc      # noqa: E402
import rollout_cases as rc      # noqa: E402


def reference_rollout(solve, groups, mass, dt, x, s, K, steps):
    """{T: q (N, 3)} for one start frame: positions ``x``, explicit state ``s``."""
    positions, out = x.copy(), {}
    for t in range(1, max(steps) + 1):
        q_next = reference_loop(solve, groups, mass, dt, s, (K,))[K]
        velocities = (q_next - positions) / dt                     # :531
        positions = q_next                                         # :532
        s = positions + dt * velocities                            # :495 of the next step
        if t in steps:
            out[t] = q_next.copy()
    return out


def record(Simulators, name, groups, rest, frames):
    N = frames.shape[1]
    mass = masses_of(N)
    solve = reference_solver(Simulators, [c for g in groups for c in g[0]], rest, mass, DT)
    case = pc.host_case(name, load=load)
    sel, steps = rc.START_FRAMES, rc.STEPS[name]
    arrays = {}
    for mode in pc.MODES:
        s, x = rc.start_state(frames, sel, mode)
        for K in pc.KS:
            q = {T: np.empty_like(x) for T in steps}
            for i in range(len(sel)):
                got = reference_rollout(solve, groups, mass, DT, x[i], s[i], K, steps)
                for T in steps:
                    q[T][i] = got[T]
            amp = rc.measure_amp(case, mode, K, max(steps))
            host = rc.rollout(case, K, max(steps), s, x)
            for T in steps:
                assert amp[T - 1] <= pc.AMP_CAP, (name, mode, K, T, amp[T - 1])
                arrays["q_%s_%d_%d" % (mode, K, T)] = q[T]
                arrays["amp_%s_%d_%d" % (mode, K, T)] = np.float64(amp[T - 1])
                print("%-28s %-10s K = %2d T = %d: amp %.3g, |host model - reference| %.3g"
                      % (name, mode, K, T, amp[T - 1], np.abs(host[T - 1] - q[T]).max()), flush=True)
    save("rollout_" + name, dt=np.float64(DT), wi=np.float64(WI), Ks=np.array(pc.KS, dtype=np.int64),
         steps=np.array(steps, dtype=np.int64), start_frames=np.array(sel, dtype=np.int64), **arrays)


def record_reduced(fixture, kind, p):
    from animsnapbases_amd import reduced
    r = load("reduced_forces_" + fixture)
    case = pc.host_case(kind, load=load)
    ms = [int(m) for m in r["ms"]]
    arrays, keep = {}, len(rc.LONG)
    for m in (ms[0], ms[-1]):
        op = reduced.reduced_operator(r["components"], r["interpol_alphas"], r["Pt"], r["interpol_alpha_ranges"], m, p,
                                      str(r["reduction"]), n_elements=r["components"].shape[1] // p)
        for mode in pc.MODES:
            for K in pc.KS:
                amp = rc.measure_amp(case, mode, K, max(rc.LONG), reduced=(0, op))
                for i, T in enumerate(rc.LONG):
                    arrays["amp_%d_%s_%d_%d" % (m, mode, K, T)] = np.float64(amp[T - 1])
                    if amp[T - 1] > pc.AMP_CAP:
                        keep = min(keep, i)
                    print("%-28s m = %2d %-10s K = %2d T = %d: amp %.3g" % ("reduced " + fixture, m, mode, K, T, amp[T - 1]), flush=True)
    steps = rc.LONG[:keep]
    arrays = {k: v for k, v in arrays.items() if int(k.rsplit("_", 1)[1]) in steps}
    print("reduced %s keeps the steps %s" % (fixture, list(steps)))
    save("rollout_reduced_" + fixture, ms=np.array([ms[0], ms[-1]], dtype=np.int64), steps=np.array(steps, dtype=np.int64), **arrays)


def reference_records(CP, Simulators):
    def build(kind, g):
        rest, el, sig = g["rest"], g["elements"], g["sigma"]
        if kind == "edge_spring":
            cs = [CP.EdgeSpringConstraint(e.tolist(), WI, rest) for e in el]
        elif kind == "tris_strain":
            cs = [CP.TriStrainConstraint(t.tolist(), WI, rest, *sig) for t in el]
        elif kind == "tets_strain":
            cs = [CP.TetStrainConstraint(t.tolist(), WI, rest, *sig) for t in el]
        else:
            cs = [CP.TetDeformationGradientConstraint(t.tolist(), WI, rest) for t in el]
        return cs, P_ROWS[kind], sparse.hstack([c._selection_matrix for c in cs]).tocsr()

    made = {}
    for kind in ("edge_spring", "tris_strain", "tets_strain", "tets_deformation_gradient"):
        g = load("cproj_" + kind)
        made[kind] = (build(kind, g), g)
        record(Simulators, kind, [made[kind][0]], g["rest"], g["frames"])
    g_t = made["tets_strain"][1]
    record(Simulators, "combined", [made["edge_spring"][0], made["tets_strain"][0]], g_t["rest"], g_t["frames"])


def main():
    CP, Simulators = import_reference_simulator()
    if "--reduced-only" not in sys.argv:
        reference_records(CP, Simulators)
    for fixture, kind in rc.REDUCED.items():
        record_reduced(fixture, kind, P_ROWS[kind])


if __name__ == "__main__":
    main()
