"""Writes tests/golden/gstep_<kind>.npz and gstep_combined.npz from the UNMODIFIED reference classes of
projective_dynamics/Constraint_projections.py (CPU only; never imported by a test).

    python tools/gen_golden_gstep.py

Inputs: the committed tests/golden/cproj_<kind>.npz (rest, elements, frames, sigma) and st_<kind>.npz / st_combined.npz (the
constraint term b).  The constraints are built with wi = 0.7 and handed, with dt = 0.5 and a fixed non-uniform mass vector,
to the reference's own ``prepare_global_matrix`` (Simulators.py:117-145), whose factorisation does every solve recorded here.
That routine keeps no matrix, so the sum of the ``get_wi_SiT_AiT_Ai_Si()`` triplets and the mass diagonal is formed here as
well; the script asserts that it is kron(A_N, I_3), symmetric, and the matrix the reference solved (residual of every solve),
and records cond(A_N).  Each file holds A_N as COO ``row`` / ``col`` /
``val`` / ``shape``, ``masses``, ``dt``, ``wi``, ``cond`` and, per frame of the fixture, the reference's global step
``q = cholesky(flatten(b + M / dt^2 s))`` (Simulators.py:145, :502-526) for both explicit states: ``q_zero`` with
s = x_f and ``q_difference`` with s = 2 x_f - x_{f-1} (x_{-1} = x_0; :495 with the velocity of :531, no external force).

``verts_bending`` has no file: the reference's ``VertBendingConstraint.get_wi_SiT_AiT_Ai_Si`` (:223-249) multiplies its (N, 1)
selection column the other way round, a 1 x 1 product that lands on vertex 0, so it does not state the matrix of its own
constraint; projections.global_matrix builds wi_v s s^T from the definition and tests/test_gstep_cpu.py checks that directly.
"""
import os
import sys
import types

import numpy as np
import scipy.sparse
import scipy.sparse.linalg

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_cproj import GOLDEN, save      # noqa: E402
from gen_reduced_forces_golden import import_reference_simulator      # noqa: E402

WI = 0.7
DT = 0.5


def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def masses_of(n):
    i = np.arange(n, dtype=np.float64)
    return 0.6 + 0.35 * np.sin(1.3 * i + 0.2) + 0.02 * (i % 5)


def reference_solver(Simulators, constraints, rest, mass, dt):
    """The unmodified ``prepare_global_matrix`` (Simulators.py:117-145) run on a bare solver object: its ``cholesky``."""
    s = object.__new__(Simulators.animSnapBasesSolver)
    s.reduced_position = False
    s.model = types.SimpleNamespace(mass=mass, positions=rest, constraints=constraints)
    s.prepare_global_matrix(types.SimpleNamespace(dt=dt))
    return s.cholesky


def triplet_matrix(constraints, mass, dt):
    """The 3N x 3N matrix those triplets sum to, put together here only to record A_N and to check the solve against it."""
    t = np.array([e for c in constraints for e in c.get_wi_SiT_AiT_Ai_Si()], dtype=np.float64)
    n3 = 3 * mass.shape[0]
    K = scipy.sparse.coo_matrix((t[:, 2], (t[:, 0].astype(np.int64), t[:, 1].astype(np.int64))), shape=(n3, n3))
    return (K + scipy.sparse.kron(scipy.sparse.diags(mass / dt ** 2), scipy.sparse.identity(3))).tocsc()


def record(Simulators, name, constraints, rest, frames, b):
    N = frames.shape[1]
    mass = masses_of(N)
    assert (mass > 0).all()
    solve = reference_solver(Simulators, constraints, rest, mass, DT)
    A3 = triplet_matrix(constraints, mass, DT)
    D = A3.toarray()
    blocks = [D[d::3, d::3] for d in range(3)]
    assert np.array_equal(blocks[0], blocks[1]) and np.array_equal(blocks[0], blocks[2])
    assert np.array_equal(np.kron(blocks[0], np.eye(3)), D)                  # no coupling between coordinates
    A_N = blocks[0]
    assert np.abs(A_N - A_N.T).max() <= 1e-15 * np.abs(A_N).max()
    cond = np.linalg.cond(A_N)
    q = {"zero": np.empty_like(frames), "difference": np.empty_like(frames)}
    worst = 0.0
    for f in range(frames.shape[0]):
        prev = frames[max(f - 1, 0)]
        for mode, s in (("zero", frames[f]), ("difference", 2.0 * frames[f] - prev)):
            rhs = b[f] + (mass / DT ** 2)[:, None] * s
            x = solve(rhs.flatten())
            worst = max(worst, np.abs(A3 @ x - rhs.flatten()).max() / np.abs(rhs).max())
            q[mode][f] = x.reshape(N, 3)
    assert worst <= 64 * np.finfo(float).eps * cond, worst                   # the recorded A_N is the matrix the reference solved
    c = scipy.sparse.coo_matrix(A_N)
    print("%-28s N = %d, cond(A_N) = %.3f" % (name, N, cond))
    save("gstep_" + name, row=c.row.astype(np.int64), col=c.col.astype(np.int64), val=c.data.astype(np.float64),
         shape=np.array(A_N.shape, dtype=np.int64), masses=mass, dt=np.float64(DT), wi=np.float64(WI), cond=np.float64(cond),
         q_zero=q["zero"], q_difference=q["difference"])


def main():
    CP, Simulators = import_reference_simulator()

    def build(kind, g):
        rest, el, sig = g["rest"], g["elements"], g["sigma"]
        if kind == "edge_spring":
            return [CP.EdgeSpringConstraint(e.tolist(), WI, rest) for e in el]
        if kind == "tris_strain":
            return [CP.TriStrainConstraint(t.tolist(), WI, rest, *sig) for t in el]
        if kind == "tets_strain":
            return [CP.TetStrainConstraint(t.tolist(), WI, rest, *sig) for t in el]
        return [CP.TetDeformationGradientConstraint(t.tolist(), WI, rest) for t in el]

    made = {}
    for kind in ("edge_spring", "tris_strain", "tets_strain", "tets_deformation_gradient"):
        g = load("cproj_" + kind)
        st = load("st_" + kind)
        assert float(st["wi"]) == WI
        made[kind] = (build(kind, g), g)
        record(Simulators, kind, made[kind][0], g["rest"], g["frames"], st["b"])
    # the two kinds of st_combined on the tetrahedra's frames
    cs_e, g_e = made["edge_spring"]
    cs_t, g_t = made["tets_strain"]
    assert np.array_equal(g_e["rest"], g_t["rest"])
    record(Simulators, "combined", cs_e + cs_t, g_t["rest"], g_t["frames"], load("st_combined")["b"])


if __name__ == "__main__":
    main()
