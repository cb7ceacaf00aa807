"""Writes tests/golden/st_<name>.npz from the UNMODIFIED reference classes of
projective_dynamics/Constraint_projections.py (CPU only; never imported by a test).

    python tools/gen_golden_st.py

Inputs: the committed tests/golden/cproj_<name>.npz (``rest``, ``elements``, ``frames``, ``sigma``).  The reference's
constraints are built with wi = 0.7 (a dropped weight cannot pass).  Each file holds ``wi``, the reference's assembly matrix
S^T (:1221-1284: column block e is the element's ``_selection_matrix``) as COO ``row`` / ``col`` / ``val`` / ``shape`` after
``tocsr()``, and ``b`` (F, N, 3) = ``assembly_ST @ stacked_p`` per frame as ``get_sum_ST_p`` computes it
(Simulators.py:643-724).  ``st_combined``: the tetrahedra of cproj_tets_strain and the edges of cproj_edge_spring on the
tetrahedra's frames, b = S_edge^T p_edge + S_tet^T p_tet in the reference's order (edge first), plus ``p_edge`` there (the
test's rounding bound needs its size).  ``st_edge_spring_collapsed``: b with the NaN row of the collapsed edge.
"""
import os
import sys

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_cproj import GOLDEN, import_reference_projections, save, stack      # noqa: E402

WI = 0.7


def load(name):
    with np.load(os.path.join(GOLDEN, "cproj_" + name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def assemble(constraints):
    """(|V|, p |elements|): column block e is constraint e's selection matrix, as the reference's add_* loops fill it."""
    return sparse.hstack([c._selection_matrix for c in constraints]).tocsr()


def forces(St, p):
    return np.stack([St @ p[f] for f in range(p.shape[0])])


def coo(St):
    St = St.tocsr()
    c = St.tocoo()
    return dict(row=c.row.astype(np.int64), col=c.col.astype(np.int64), val=c.data.astype(np.float64),
                shape=np.array(St.shape, dtype=np.int64))


def main():
    CP = import_reference_projections()
    made = {}

    def build(kind, g):
        rest, el, sig = g["rest"], g["elements"], g["sigma"]
        if kind == "edge_spring":
            return [CP.EdgeSpringConstraint(e.tolist(), WI, rest) for e in el], 1
        if kind == "tris_strain":
            return [CP.TriStrainConstraint(t.tolist(), WI, rest, *sig) for t in el], 2
        if kind == "tets_strain":
            return [CP.TetStrainConstraint(t.tolist(), WI, rest, *sig) for t in el], 3
        return [CP.TetDeformationGradientConstraint(t.tolist(), WI, rest) for t in el], 3

    for kind in ("edge_spring", "tris_strain", "tets_strain", "tets_deformation_gradient"):
        g = load(kind)
        cs, p = build(kind, g)
        St = assemble(cs)
        P = stack(cs, g["frames"], p)
        assert np.array_equal(P, g["expected"])               # get_pi does not depend on wi
        assert St.shape == (g["rest"].shape[0], P.shape[1])
        made[kind] = (St, g)
        save("st_" + kind, wi=np.float64(WI), b=forces(St, P), **coo(St))

    for tag in ("grid", "closed"):
        g = load("verts_bending_" + tag)
        mesh = CP.DeformableMesh(g["rest"].copy(), g["elements"])
        mesh.add_vertex_bending_constraint(WI)
        assert np.array_equal(np.array(mesh.verts_bending_indicies), g["indices"])
        P = stack(mesh.verts_bending_constraints, g["frames"], 1)
        assert np.array_equal(P, g["expected"])
        St = mesh.verts_bending_assembly_ST.tocsr()
        save("st_verts_bending_" + tag, wi=np.float64(WI), b=forces(St, P), **coo(St))

    # ---- two kinds on one animation: the tetrahedra's frames, edge first (the order of get_sum_ST_p)
    St_e, g_e = made["edge_spring"]
    St_t, g_t = made["tets_strain"]
    assert np.array_equal(g_e["rest"], g_t["rest"])
    fr, E = g_t["frames"], g_e["elements"]
    assert (np.linalg.norm(fr[:, E[:, 0]] - fr[:, E[:, 1]], axis=2) > 0).all()
    p_edge = stack(build("edge_spring", g_e)[0], fr, 1)
    b = np.zeros((fr.shape[0], fr.shape[1], 3))
    for f in range(fr.shape[0]):
        rhs = np.zeros((fr.shape[1], 3))
        rhs += St_e @ p_edge[f]
        rhs += St_t @ g_t["expected"][f]
        b[f] = rhs
    save("st_combined", wi=np.float64(WI), b=b, p_edge=p_edge)

    # ---- the collapsed edge: NaN reaches exactly the two vertices of that edge in that frame
    g = load("edge_spring_collapsed")
    cs, _ = build("edge_spring", g)
    St = assemble(cs)
    P = stack(cs, g["frames"], 1)
    assert np.array_equal(np.isnan(P), np.isnan(g["expected"]))
    b = forces(St, P)
    bad = np.isnan(b).any(axis=2)
    assert bad.sum() == 2 and sorted(np.flatnonzero(bad[2]).tolist()) == sorted(g["elements"][3].tolist())
    save("st_edge_spring_collapsed", wi=np.float64(WI), b=b, **coo(St))


if __name__ == "__main__":
    main()
