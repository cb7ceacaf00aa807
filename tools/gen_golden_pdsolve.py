"""Writes tests/golden/pdsolve_<kind>.npz, pdsolve_combined.npz and pdsolve_reduced_<fixture>.npz (CPU only; never imported
by a test).

    python tools/gen_golden_pdsolve.py [--reduced-only]

pdsolve_<name>: what the UNMODIFIED reference's own loop (Simulators.py:506-526) produces.  The constraints are the
reference's classes, built with wi = 0.7; ``cholesky`` is the factorisation its ``prepare_global_matrix`` (:117-145) leaves on
a bare solver object (dt = 0.5, the mass vector of tools/gen_golden_gstep.py); the b of every iteration is
``assembly_ST @ stacked_p`` of the reference's ``get_pi`` at the current q, the kinds in the order of ``get_sum_ST_p``
(:643-724), plus the mass term of :502-504.  Per frame of the cproj fixture and per explicit state -- ``zero``: s = x_f,
``difference``: s = 2 x_f - x_{f-1} (x_{-1} = x_0) -- the loop starts at q = s and ``q_<mode>_<K>`` (F, N, 3) is q after
K in {1, 3, 10} iterations.  ``amp_<mode>_<K>``: the amplification tests/pdsolve_cases.py measures ON ITS HOST MODEL
(perturbed starts; its docstring), which the tests' bound B_K uses.

pdsolve_reduced_<fixture>: ``amp_<m>_<mode>_<K>`` of the host model with the kind reduced to m components, for the smallest
and largest m of tests/golden/reduced_forces_<fixture>.npz (the reduced solve has no reference run; the tests compare the
device with the host route)."""
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
from gen_reduced_forces_golden import import_reference_simulator      # noqa: E402
import pdsolve_cases as pc      # noqa: E402

P_ROWS = {"edge_spring": 1, "tris_strain": 2, "tets_strain": 3, "tets_deformation_gradient": 3}


def reference_loop(solve, groups, mass, dt, s, Ks):
    """Simulators.py:500-526 for one frame with explicit state ``s`` (N, 3): {K: q (N, 3)}.  ``groups``: per kind the
    reference's constraints, their rows per element and their assembly matrix."""
    N = s.shape[0]
    dt2_inv = 1.0 / (dt * dt)
    sn = s.flatten()
    masses = np.zeros(3 * N)
    for i in range(N):
        masses[3 * i:3 * i + 3] = dt2_inv * mass[i] * sn[3 * i:3 * i + 3]
    q = sn.copy()
    out = {}
    for it in range(1, max(Ks) + 1):
        b = np.zeros((N, 3))
        for cs, p, St in groups:
            stacked = np.zeros((St.shape[1], 3))
            for i, c in enumerate(cs):
                stacked[p * i:p * i + p, :] = c.get_pi(q)
            b += St @ stacked
        b += masses.reshape(N, 3)
        q = solve(b.flatten())
        if it in Ks:
            out[it] = q.reshape(N, 3).copy()
    return out


def record(Simulators, name, groups, rest, frames):
    F, N = frames.shape[:2]
    mass = masses_of(N)
    solve = reference_solver(Simulators, [c for g in groups for c in g[0]], rest, mass, DT)
    arrays = {}
    case = pc.host_case(name, load=load)
    for mode in pc.MODES:
        s = pc.explicit_state(frames, range(F), mode)
        q = {K: np.empty_like(frames) for K in pc.KS}
        for f in range(F):
            got = reference_loop(solve, groups, mass, DT, s[f], pc.KS)
            for K in pc.KS:
                q[K][f] = got[K]
        amp = pc.measure_amp(case, mode)
        host = pc.model(case, range(F), mode, pc.KS)
        for K in pc.KS:
            assert amp[K] <= pc.AMP_CAP, (name, mode, K, amp[K])
            arrays["q_%s_%d" % (mode, K)] = q[K]
            arrays["amp_%s_%d" % (mode, K)] = np.float64(amp[K])
            print("%-28s %-10s K = %2d: amp %.3g, |host model - reference| %.3g" % (name, mode, K, amp[K], np.abs(host[K] - q[K]).max()))
    save("pdsolve_" + name, dt=np.float64(DT), wi=np.float64(WI), Ks=np.array(pc.KS, dtype=np.int64), **arrays)


def record_reduced(fixture, kind, p):
    from animsnapbases_amd import reduced
    r = load("reduced_forces_" + fixture)
    case = pc.host_case(kind, load=load)
    ms = [int(m) for m in r["ms"]]
    arrays = {}
    for m in (ms[0], ms[-1]):
        op = reduced.reduced_operator(r["components"], r["interpol_alphas"], r["Pt"], r["interpol_alpha_ranges"], m, p,
                                      str(r["reduction"]), n_elements=r["components"].shape[1] // p)
        for mode in pc.MODES:
            amp = pc.measure_amp(case, mode, reduced=(0, op))
            for K in pc.KS:
                assert amp[K] <= pc.AMP_CAP, (fixture, m, mode, K, amp[K])
                arrays["amp_%d_%s_%d" % (m, mode, K)] = np.float64(amp[K])
                print("%-28s m = %2d %-10s K = %2d: amp %.3g" % ("reduced " + fixture, m, mode, K, amp[K]))
    save("pdsolve_reduced_" + fixture, ms=np.array([ms[0], ms[-1]], dtype=np.int64), **arrays)


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
    assert np.array_equal(made["edge_spring"][1]["rest"], g_t["rest"])
    record(Simulators, "combined", [made["edge_spring"][0], made["tets_strain"][0]], g_t["rest"], g_t["frames"])


def main():
    CP, Simulators = import_reference_simulator()
    if "--reduced-only" not in sys.argv:
        reference_records(CP, Simulators)
    record_reduced("tets_deim", "tets_strain", 3)
    record_reduced("tris_blocks", "tris_strain", 2)


if __name__ == "__main__":
    main()
