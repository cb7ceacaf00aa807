"""CPU: ``projections.global_matrix`` -- A_N = M / dt^2 + sum_i w_i S_i^T S_i assembled from the rest tables of ``build_setup``
-- against the system matrix the unmodified reference assembles from ``get_wi_SiT_AiT_Ai_Si`` (tools/gen_golden_gstep.py;
Simulators.py:117-145), built there with wi = 0.7, dt = 0.5 and a non-uniform mass vector.

Tolerance: 1e-13 of the matrix's largest entry (every entry is a short sum of products of rest-table entries, held to that
figure by tests/test_cproj_cpu.py, times wi times a rest area / volume).

``verts_bending`` has no reference matrix (tools/gen_golden_gstep.py says why); its term is checked against the definition
wi_v s s^T summed densely from the fixture's own cotangent weights."""
import types

import numpy as np
import pytest
from scipy import sparse

from conftest import load_golden

from animsnapbases_amd import projections as proj
from animsnapbases_amd.posSnapshots import posSnapshots

KINDS = ["edge_spring", "tris_strain", "tets_strain", "tets_deformation_gradient"]
BENDING = ["verts_bending_grid", "verts_bending_closed"]


def _case(kind):
    g, z = load_golden("cproj_" + kind), load_golden("gstep_" + kind)
    ref = sparse.coo_matrix((z["val"], (z["row"], z["col"])), shape=tuple(z["shape"])).toarray()
    return g, z, ref, proj.build_setup(kind, g["elements"], g["rest"])


def _check(A, ref):
    N = ref.shape[0]
    assert sparse.isspmatrix_csr(A) and A.shape == (N, N)
    assert A.has_sorted_indices and all((np.diff(A.indices[A.indptr[v]:A.indptr[v + 1]]) > 0).all() for v in range(N))
    err = np.abs(A.toarray() - ref).max() / np.abs(ref).max()
    print("N = %d, %d entries, max error / largest entry %.3g" % (N, A.nnz, err))
    assert err <= 1e-13


@pytest.mark.parametrize("kind", KINDS)
def test_matches_the_reference(kind):
    g, z, ref, setup = _case(kind)
    assert float(z["wi"]) == 0.7 and float(z["dt"]) == 0.5 and np.ptp(z["masses"]) > 0
    _check(proj.global_matrix([(setup, float(z["wi"]))], g["rest"].shape[0], z["masses"], float(z["dt"])), ref)


def test_two_kinds_match_the_reference_and_add_up():
    g_e, z, ref, edge = _case("edge_spring")
    g_t, z_t, _, tets = _case("tets_strain")
    z = load_golden("gstep_combined")
    ref = sparse.coo_matrix((z["val"], (z["row"], z["col"])), shape=tuple(z["shape"])).toarray()
    N, m, dt = g_t["rest"].shape[0], z["masses"], float(z["dt"])
    both = proj.global_matrix([(edge, 0.7), (tets, 0.7)], N, m, dt)
    _check(both, ref)
    mass = np.diag(m / dt ** 2)
    parts = [proj.global_matrix([(s, 0.7)], N, m, dt).toarray() - mass for s in (edge, tets)]
    assert np.abs(both.toarray() - mass - parts[0] - parts[1]).max() <= 4 * np.finfo(float).eps * np.abs(ref).max()
    swapped = proj.global_matrix([(tets, 0.7), (edge, 0.7)], N, m, dt)
    assert np.abs(swapped.toarray() - both.toarray()).max() <= 4 * np.finfo(float).eps * np.abs(ref).max()


@pytest.mark.parametrize("kind", KINDS + BENDING)
def test_symmetric_and_linear_in_wi(kind):
    g = load_golden("cproj_" + kind)
    N = g["rest"].shape[0]
    setup = proj.build_setup("verts_bending" if kind in BENDING else kind, g["elements"], g["rest"])
    # masses far below the constraint terms: A - M then loses nothing, and a weight so small that every contribution lies
    # under the reference's drop threshold of 1e-12 must still come out in proportion
    m = 1e-20 * (0.5 + 0.1 * np.arange(N))
    mass = np.diag(m * (1.0 / (0.25 * 0.25)))
    one = proj.global_matrix([(setup, 1.0)], N, m, 0.25)
    assert abs(one - one.T).max() == 0.0
    K1 = one.toarray() - mass
    assert np.abs(K1).max() > 1e-3
    assert np.linalg.eigvalsh(K1).min() >= -1e-12 * np.abs(K1).max()        # a sum of Gram matrices
    assert np.abs(K1.sum(axis=1)).max() <= 1e-12 * np.abs(K1).max()         # translations cost nothing
    # an entry sums at most one contribution per element, each rounded at its own size, in both matrices
    terms = 2 * (setup.n_elem + 4)
    for wi in (4.0, 0.7, 1e-14):
        Kw = proj.global_matrix([(setup, wi)], N, m, 0.25).toarray() - mass
        assert np.abs(Kw - wi * K1).max() <= terms * np.finfo(float).eps * (np.abs(mass).max() + wi * np.abs(K1).max())
    zero = proj.global_matrix([(setup, 0.0)], N, m, 0.25).toarray()
    assert np.array_equal(zero, mass)


@pytest.mark.parametrize("name", BENDING)
def test_bending_term_is_the_weighted_outer_product_of_the_selection_rows(name):
    g = load_golden("cproj_" + name)
    N = g["rest"].shape[0]
    setup = proj.build_setup("verts_bending", g["elements"], g["rest"])
    wi, m = 0.7, np.ones(N)
    K = np.zeros((N, N))
    ptr, nb, w = g["star_ptr"], g["star_idx"], g["weights"]
    for i, v in enumerate(g["indices"]):
        s = np.zeros(N)
        s[v] = w[ptr[i]:ptr[i + 1]].sum()
        for e in range(ptr[i], ptr[i + 1]):
            s[nb[e]] -= w[e]
        K += wi * setup.parts["voronoi_area"][i] * np.outer(s, s)
    A = proj.global_matrix([(setup, wi)], N, m, 1.0).toarray() - np.eye(N)
    assert np.abs(A - K).max() <= 1e-13 * np.abs(K).max()
    # ... which is what S^T holds: A = S^T diag(1 / wi_v) S for the weighted operator of assembly_ST
    St = proj.assembly_ST(setup, N, wi).toarray()
    assert np.abs(St @ np.diag(1.0 / (wi * setup.parts["voronoi_area"])) @ St.T - K).max() <= 1e-13 * np.abs(K).max()


def test_refusals():
    g, z, _, setup = _case("tets_strain")
    N, m = g["rest"].shape[0], z["masses"]
    ok = proj.global_matrix([(setup, 0.7)], N, m, 0.5)
    assert ok.shape == (N, N)
    for dt in (0.0, -0.5, np.nan, np.inf, None, "fast"):
        with pytest.raises(ValueError):
            proj.global_matrix([(setup, 0.7)], N, m, dt)
    bad = m.copy()
    for masses in (m[:-1], m[None, :], np.concatenate([m, [1.0]])):
        with pytest.raises(ValueError):
            proj.global_matrix([(setup, 0.7)], N, masses, 0.5)
    for v in (0.0, -1.0, np.nan, np.inf):
        bad = m.copy()
        bad[3] = v
        with pytest.raises(ValueError):
            proj.global_matrix([(setup, 0.7)], N, bad, 0.5)
    for wi in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            proj.global_matrix([(setup, wi)], N, m, 0.5)
    for specs in ([], (), None):
        with pytest.raises(ValueError):
            proj.global_matrix(specs, N, m, 0.5)
    with pytest.raises(ValueError):
        proj.global_matrix([setup], N, m, 0.5)                              # not a (setup, wi) pair
    with pytest.raises(ValueError):
        proj.global_matrix([(setup, 0.7)], N - 1, m[:-1], 0.5)              # an element outside the matrix


def _bare(multi):
    snaps = posSnapshots.__new__(posSnapshots)
    snaps._comm = types.SimpleNamespace(multi=multi)
    return snaps


def test_several_ranks_are_refused():
    g = load_golden("cproj_tets_strain")
    kinds = [dict(kind="tets_strain", elements=g["elements"])]
    snaps = _bare(True)
    with pytest.raises(NotImplementedError):
        snaps.global_solve_setup(kinds, 0.5, np.ones(g["rest"].shape[0]))
    with pytest.raises(NotImplementedError):
        snaps.global_solve(None)
    with pytest.raises(NotImplementedError):
        snaps.global_step(kinds, 0.5, np.ones(g["rest"].shape[0]))
    with pytest.raises(NotImplementedError):
        snaps.reduced_global_step_errors("tets_strain", {}, [1], 0.5, np.ones(g["rest"].shape[0]))


def test_arguments_checked_before_the_device_is_touched():
    snaps = _bare(False)
    snaps.mass, snaps.global_matrix = None, None
    with pytest.raises(ValueError, match="masses"):
        snaps.global_step([dict(kind="edge_spring", elements=np.array([[0, 1]]))], 0.5)
    with pytest.raises(ValueError, match="velocity"):
        snaps.global_step([], 0.5, np.ones(4), velocity="leapfrog")
    with pytest.raises(ValueError, match="gravity"):
        snaps.global_step([], 0.5, np.ones(4), gravity=(0.0, np.nan, 0.0))
    with pytest.raises(ValueError, match="dt"):
        snaps.global_step([], 0.0, np.ones(4))
    with pytest.raises(ValueError, match="global_solve_setup"):
        snaps.global_solve(None)
