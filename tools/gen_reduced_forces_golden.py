"""Writes tests/golden/reduced_forces_<name>.npz from the UNMODIFIED reference simulator: ``prepare_reduced_group``,
``prepare_reduced_verts_bending`` and ``get_group_reduced_term`` of projective_dynamics/Simulators.py (:157-255, :366-399) on
the reference's constraint objects (CPU only; never imported by a test).

    python tools/gen_reduced_forces_golden.py

Inputs: the committed tests/golden/cproj_<kind>.npz (``rest``, ``elements``, ``frames``, ``expected``, ``sigma``); the box
builds its own mesh and frames.  The constraints carry wi = 0.7.  The bases are NumPy restatements, in this file, of the
reference's own routines on the fixture's ``expected`` projections: ``pod_vectorized`` (constraintsComponents.py:298-320) with
``deim`` points (:797-860), and for the blocks a per-coordinate POD of K p vectors with block-DEIM points (the element with
the largest residual of the next p vectors).  They are written through the four keys of ``store_components_n_interpol_points``
into a temporary directory, from where the reference loads them.

Each file: the four basis keys, ``reduction``, ``wi``, ``ms``, per m ``b_ref_<m>`` (F, N, 3) -- ``get_group_reduced_term`` of
every frame -- ``Pt_<m>`` and ``alphas_<m>`` as the reference returns them, ``la_<m>`` (3,) and ``cond_<m>`` (3,) of the
reference's AtA_d + la_d I, and ``projecting_mat_<m>`` (N, m p, 3) for the largest m.  ``box`` also holds ``rest``, ``elements``,
``frames``, ``sigma``, ``expected_pt`` (F, |Pt|, 3): the reference's projections at the rows Pt of the largest m, and the
reference's S^T as COO ``st_row`` / ``st_col`` / ``st_val``.

Condition on the fixtures (asserted here, recomputed by the tests; not a tolerance): cond(AtA_d + la_d I) <= 1e6 for every
stored m and d.
"""
import os
import sys
import tempfile
import types

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_cproj import GOLDEN, SIGMA, animate, box_tets, import_reference_projections, save, tet_F, tet_conditions   # noqa: E402
from oracle.ref_import import REF_ROOT      # noqa: E402

WI = 0.7
COND_CAP = 1e6
FILE = "components_interpol_alphas_interpol_verts_interpol_alpha_ranges.npz"


def load(name):
    with np.load(os.path.join(GOLDEN, "cproj_" + name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def import_reference_simulator():
    CP = import_reference_projections()
    import Simulators
    assert os.path.realpath(Simulators.__file__).startswith(os.path.realpath(REF_ROOT))
    return CP, Simulators


# ------------------------------------------------------------------ bases (restated from the reference's routines)
def pod_vectorized(P, K):
    """constraintsComponents.py:298-320: svd of (F, ep, 3).reshape(F, -1).T, comps = U.T.reshape(-1, ep, 3)[:K]."""
    F = P.shape[0]
    U = np.linalg.svd(P.reshape(F, -1).T, full_matrices=False)[0]
    return np.ascontiguousarray(U.T.reshape(-1, P.shape[1], 3)[:K])


def deim(comps, p):
    """constraintsComponents.py:797-860."""
    bases = comps.swapaxes(0, 1)
    K = comps.shape[0]
    Pt, alphas, ranges = [], [], []
    for k in range(K):
        vk = bases[:, k, :]
        if k == 0:
            r = vk
        else:
            c = np.empty(vk.shape)
            for i in range(3):
                c[:, i] = bases[:, :k, i] @ np.linalg.lstsq(bases[Pt, :k, i], vk[Pt, i], rcond=None)[0]
            r = c - vk
        idx = int(np.argmax((r ** 2).sum(axis=1)))
        Pt.append(idx)
        alphas.append(idx // p)
        ranges.append(k + 1)
    return np.array(Pt), np.array(alphas), np.array(ranges)


def pod_blocks(P, K, p):
    """K p vectors per coordinate: the leading left singular vectors of (F, ep).T, coordinate by coordinate."""
    comps = np.empty((K * p, P.shape[1], 3))
    for d in range(3):
        comps[:, :, d] = np.linalg.svd(P[:, :, d].T, full_matrices=False)[0][:, :K * p].T
    return comps


def block_deim(comps, p, extra=0):
    """Per block k of p vectors: the element (not taken yet) whose p rows carry the largest residual of the block after the
    least-squares interpolation at the rows taken so far; ``extra`` more elements per block the same way."""
    bases = comps.swapaxes(0, 1)
    K = comps.shape[0] // p
    alphas, ranges, rows = [], [], []
    for k in range(K):
        for _ in range(1 + extra):
            vk = bases[:, k * p:(k + 1) * p, :]
            if rows and k > 0:
                r = np.empty(vk.shape)
                for i in range(3):
                    r[:, :, i] = bases[:, :k * p, i] @ np.linalg.lstsq(bases[rows, :k * p, i], vk[rows, :, i], rcond=None)[0] - vk[:, :, i]
            else:
                r = vk
            e = (r ** 2).sum(axis=(1, 2)).reshape(-1, p).sum(axis=1)
            e[alphas] = -1.0
            a = int(np.argmax(e))
            alphas.append(a)
            rows += [a * p + l for l in range(p)]
        ranges.append(len(alphas))
    alphas = np.array(alphas)
    return (alphas[:, None] * p + np.arange(p)[None, :]).reshape(-1), alphas, np.array(ranges)


# ------------------------------------------------------------------ the reference run
def new_solver(Simulators, reduction):
    s = object.__new__(Simulators.animSnapBasesSolver)
    s.constraint_projection_reduction_type = reduction
    s.reduced_position = False
    return s


def reference_group(Simulators, constraints, St, basis, group, reduction, p, ms, frames):
    """b_ref, la, cond and projecting_mat per m through prepare_reduced_group / get_group_reduced_term."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, group))
        np.savez(os.path.join(tmp, group, FILE), **basis)
        for m in ms:
            s = new_solver(Simulators, reduction)
            alphas, Pt, pm, solvers = s.prepare_reduced_group(True, True, group, m, p, St, tmp, FILE)
            # la is local to the reference's routine: its expressions (:205-209) on the PtV_T it returns
            PtV_T = np.stack([sv[1] for sv in solvers], axis=2)         # (mp, |Pt|, 3)
            AtA = np.einsum('nai,ami->nmi', PtV_T, PtV_T.swapaxes(0, 1))
            la = 1e-8 * np.trace(AtA) / AtA.shape[0]
            cond = np.array([np.linalg.cond(AtA[:, :, d] + la[d] * np.eye(AtA.shape[0])) for d in range(3)])
            b = np.stack([s.get_group_reduced_term(frames[f].reshape(-1), constraints, p, alphas, Pt, pm, solvers)
                          for f in range(frames.shape[0])])
            out[m] = dict(b=b, la=la, cond=cond, pm=pm, alphas=np.asarray(alphas), Pt=np.asarray(Pt))
    return out


def reference_bending(Simulators, mesh, basis, ms, frames):
    out = {}
    St = mesh.verts_bending_assembly_ST
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "verts_bending"))
        np.savez(os.path.join(tmp, "verts_bending", FILE), **basis)
        for m in ms:
            s = new_solver(Simulators, "deim_pca_blocks")       # (a 1-row block: the row form indexes get_pi's (3,) twice)
            s.model = types.SimpleNamespace(has_verts_bending_constraints=True, verts_bending_assembly_ST=St)
            s.reduced_verts_bending = True
            s.vert_bending_num_components, s.vert_bending_row_dim = m, 1
            s.cholesky_list_verts_bending = []
            s.prepare_reduced_verts_bending(tmp, FILE)
            Pt, pm, solvers = s.mapped_indices_verts_bending_Pt, s.projecting_mat_verts_bending, s.cholesky_list_verts_bending
            A = [sv[1].T for sv in solvers]
            cond = np.array([np.linalg.cond(a.T @ a) for a in A])
            b = np.stack([s.get_group_reduced_term(frames[f].reshape(-1), mesh.verts_bending_constraints, 1, Pt, Pt, pm, solvers)
                          for f in range(frames.shape[0])])
            out[m] = dict(b=b, la=np.zeros(3), cond=cond, pm=pm, alphas=np.asarray(Pt), Pt=np.asarray(Pt))
    return out


def write(name, basis, reduction, runs, **more):
    ms = sorted(runs)
    arrays = dict(basis, reduction=np.array(reduction), wi=np.float64(WI), ms=np.array(ms, dtype=np.int64))
    for m in ms:
        r = runs[m]
        assert (r["cond"] <= COND_CAP).all(), (name, m, r["cond"])
        assert np.isfinite(r["b"]).all()
        arrays["b_ref_%d" % m], arrays["la_%d" % m], arrays["cond_%d" % m] = r["b"], r["la"], r["cond"]
        arrays["Pt_%d" % m], arrays["alphas_%d" % m] = r["Pt"].astype(np.int64), r["alphas"].astype(np.int64)
        print("%s m = %d: |Pt| = %d, cond %s" % (name, m, len(r["Pt"]), np.array2string(r["cond"], precision=3)))
    arrays["projecting_mat_%d" % ms[-1]] = runs[ms[-1]]["pm"]
    arrays.update(more)
    save("reduced_forces_" + name, **arrays)


def basis_dict(comps, Pt, alphas, ranges):
    return {"components": comps, "interpol_alphas": np.asarray(alphas, dtype=np.int64), "Pt": np.asarray(Pt, dtype=np.int64),
            "interpol_verts": np.zeros(0, dtype=np.int64), "interpol_alpha_ranges": np.asarray(ranges, dtype=np.int64)}


def assemble(constraints):
    return sparse.hstack([c._selection_matrix for c in constraints]).tocsr()


def main():
    CP, Simulators = import_reference_simulator()

    # ---- tets_deim: the tetrahedra of cproj_tets_strain, vectorised POD (K = 20) + DEIM rows
    g = load("tets_strain")
    cs = [CP.TetStrainConstraint(t.tolist(), WI, g["rest"], *g["sigma"]) for t in g["elements"]]
    comps = pod_vectorized(g["expected"], 20)
    basis = basis_dict(comps, *deim(comps, 3))
    runs = reference_group(Simulators, cs, assemble(cs), basis, "tets_strain", "deim_pod_vectorized", 3, (1, 6, 17), g["frames"])
    write("tets_deim", basis, "deim_pod_vectorized", runs)

    # ---- tris_blocks: the triangles of cproj_tris_strain, p = 2, whole blocks
    g = load("tris_strain")
    cs = [CP.TriStrainConstraint(t.tolist(), WI, g["rest"], *g["sigma"]) for t in g["elements"]]
    comps = pod_blocks(g["expected"], 8, 2)
    basis = basis_dict(comps, *block_deim(comps, 2, extra=1))
    runs = reference_group(Simulators, cs, assemble(cs), basis, "tris_strain", "geom_pca_blocks_withSt", 2, (3, 8), g["frames"])
    write("tris_blocks", basis, "geom_pca_blocks_withSt", runs)

    # ---- bending: the closed mesh, every vertex constrained
    g = load("verts_bending_closed")
    mesh = CP.DeformableMesh(g["rest"].copy(), g["elements"])
    mesh.add_vertex_bending_constraint(WI)
    assert np.array_equal(np.array(mesh.verts_bending_indicies), g["indices"])
    comps = pod_vectorized(g["expected"], 12)
    basis = basis_dict(comps, *deim(comps, 1))
    runs = reference_bending(Simulators, mesh, basis, (2, 9), g["frames"])
    write("bending", basis, "deim_pod", runs)

    # ---- box: 9 x 5 x 3 vertices (N = 135 > 128), 24 frames
    rng = np.random.default_rng(20250311)
    rest, tets = box_tets(9, 5, 3, 0.25)
    frames = animate(rest, 24, rng, 0.004)
    assert tet_conditions(tet_F(rest, tets, frames)).all()
    cs = [CP.TetStrainConstraint(t.tolist(), WI, rest, *SIGMA) for t in tets]
    ms = (5, 10)
    P = np.zeros((frames.shape[0], 3 * len(cs), 3))
    for f in range(frames.shape[0]):
        for i, c in enumerate(cs):
            P[f, 3 * i:3 * i + 3] = c.get_pi(frames[f].reshape(-1))
    comps = pod_vectorized(P, 10)
    basis = basis_dict(comps, *deim(comps, 3))
    St = assemble(cs)
    runs = reference_group(Simulators, cs, St, basis, "tets_strain", "deim_pod", 3, ms, frames)
    pt_all = runs[ms[-1]]["Pt"]
    c = St.tocoo()
    write("box", basis, "deim_pod", runs, rest=rest, elements=tets, frames=frames, sigma=np.array(SIGMA),
          expected_pt=np.ascontiguousarray(P[:, pt_all]), st_row=c.row.astype(np.int32), st_col=c.col.astype(np.int32),
          st_val=c.data.astype(np.float64))


if __name__ == "__main__":
    main()
