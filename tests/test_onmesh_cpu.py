"""CPU: the NumPy restatement of the on-mesh accuracy measures (tests/onmesh_model.py), the host vertex-star CSR of the product
(utils.vertex_star_csr), the CSV header, and the assumptions the tolerances of tests/test_gpu_onmesh.py rest on."""
import numpy as np
import pytest

import onmesh_cases as oc
import onmesh_model as om


@pytest.mark.parametrize("subdiv", [0, 1])
def test_icosphere_normals_are_radial(subdiv):
    # every vertex of these two lies on a 5-fold or a 2-fold axis of the mesh: the area-weighted sum is radial exactly
    V, T = om.icosphere(subdiv)
    assert V.shape[0] == (12, 42)[subdiv] and T.shape[0] == (20, 80)[subdiv]
    n = om.per_vertex_normals(V, T)
    assert np.abs(n - V).max() <= 1e-12


def test_flat_grid_normals_and_zero_angle():
    V, T = om.grid_mesh(7, 9)
    n = om.per_vertex_normals(V, T)
    assert np.array_equal(n, np.tile([0.0, 0.0, 1.0], (V.shape[0], 1)))
    ang = om.angle_between_row_vectors(n, om.per_vertex_normals(V.copy(), T))
    assert np.array_equal(ang, np.zeros(V.shape[0]))
    acc = om.compute_accuracy(V[None], V[None].copy(), T, 0, 1, 1)
    assert np.array_equal(acc["accum_angle"], np.zeros(V.shape[0])) and np.array_equal(acc["accum_norm"], np.zeros(V.shape[0]))


def test_vertex_star_csr_equals_brute_force():
    from animsnapbases_amd.utils import vertex_star_csr
    rng = np.random.default_rng(0)
    # a fan of 70 triangles around vertex 0 (valence > 64), random triangles, a repeated corner, vertex 80 in no triangle
    fan = np.array([(0, 1 + i, 2 + i) for i in range(70)])
    rand = rng.integers(1, 80, size=(40, 3))
    tris = np.concatenate([fan, rand, [[5, 5, 9]]])[rng.permutation(111)]
    n = 82
    ptr, star = vertex_star_csr(tris, n)
    bptr, bstar = om.star_csr_brute(tris, n)
    assert ptr.dtype == np.int64 and star.dtype == np.int64
    assert np.array_equal(ptr, bptr) and np.array_equal(star, bstar)
    assert ptr[1] - ptr[0] >= 70 and ptr[81] == ptr[80] == ptr[82]
    for mesh in (om.grid_mesh(5, 4), om.icosphere(1)):
        V, T = mesh
        a, b = vertex_star_csr(T, V.shape[0]), om.star_csr_brute(T, V.shape[0])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    e = vertex_star_csr(np.zeros((0, 3), dtype=np.int64), 3)
    assert e[0].tolist() == [0, 0, 0, 0] and e[1].shape == (0,)
    with pytest.raises(ValueError):
        vertex_star_csr(np.array([[0, 1, 3]]), 3)


def test_csv_header_is_the_reference_list():
    from animsnapbases_amd.utils import ON_MESH_HEADER
    # generate_figures/onMesh_accuracyMeasures.py:95-98, character for character ("accum_norm_meann" included)
    assert ",".join(ON_MESH_HEADER) == ("numComponent,norm_error_min,norm_error_mean,norm_error_max,norm_error_sum,"
                                       "angle_error_min,angle_error_mean,angle_error_max,angle_error_sum,"
                                       "accum_norm_min,accum_norm_meann,accum_norm_max,"
                                       "accum_angle_min,accum_angle_mean,accum_angle_max")
    assert ON_MESH_HEADER == om.HEADER and len(ON_MESH_HEADER) == 15


def test_denominator_uses_frame_end_minus_frame_start():
    assert om.denominator(5, 200, 3000) == np.sqrt(3 * 195 * 3000)
    rng = np.random.default_rng(1)
    V, T = om.grid_mesh(4, 5)
    full = V[None] + 0.01 * rng.normal(size=(12, V.shape[0], 3))
    red = full + 0.01 * rng.normal(size=full.shape)
    a = om.compute_accuracy(full, red, T, 2, 11, 3)               # 3 frames visited, frame_end - frame_start = 9
    assert a["frame_err"].shape == (3, V.shape[0])
    d = np.sqrt(3 * 9 * V.shape[0])
    ref = ((full[5] - red[5]) ** 2).sum(axis=1) / (full[5] ** 2).sum(axis=1) / d
    assert np.array_equal(a["frame_err"][1], ref)
    assert a["mesh_err"][1] == np.linalg.norm(full[5] - red[5]) / np.linalg.norm(full[5]) / d


@pytest.mark.parametrize("name", sorted(oc.CASES))
def test_gpu_case_inputs_are_well_conditioned(name):
    """What the tolerances of the GPU tests assume, on their own inputs (selected frames): |x|^2 >= 1e-6 everywhere, the
    shortest un-normalised full-mesh vertex normal far above the rounding of its sum, no triangle folded over."""
    spec, F, K, std, mw, rest_shape, (fs, fe, fj), rs, nm = oc.CASES[name]
    verts, tris, mass = oc.make_case(name)
    rest, _, edge = oc.mesh_of(spec)
    n_rest = om.per_vertex_normals(rest, tris)
    for f in list(range(fs, fe, fj))[:40]:
        v = verts[f]
        assert (v ** 2).sum(axis=1).min() >= 1e-6
        n = om.per_vertex_normals(v, tris, normalise=False)
        ln = np.linalg.norm(n, axis=1)
        assert ln.min() >= 0.1 * edge * edge, (f, ln.min())          # ~ one triangle's area; rounding is ~1e-16 |x| edge
        assert np.einsum('ij,ij->i', n / ln[:, None], n_rest).min() > 0.5
