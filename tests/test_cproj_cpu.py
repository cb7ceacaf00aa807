"""CPU: the host set-up of the constraint projections (animsnapbases_amd/projections.py) against fixtures written by the
unmodified reference classes (tools/gen_golden_cproj.py; projective_dynamics/Constraint_projections.py), and the refusals of
``posSnapshots.constraint_projections``, which all happen before the device is touched.

Tables: 1e-13 relative, measured per element against the largest magnitude of that element's table (an entry that is an exact
zero of the reference, e.g. an off-diagonal of DmInv on the axis-aligned box, has no relative error of its own).  The star
order and the constrained vertices are integers and must be equal."""
import contextlib
import io
import types

import numpy as np
import pytest

from conftest import load_golden
from animsnapbases_amd import projections as pr

TABLE_TOL = 1e-13

FIXTURES = [("edge_spring", "cproj_edge_spring"), ("tris_strain", "cproj_tris_strain"), ("tets_strain", "cproj_tets_strain"),
            ("tets_deformation_gradient", "cproj_tets_deformation_gradient"), ("verts_bending", "cproj_verts_bending_grid"),
            ("verts_bending", "cproj_verts_bending_closed")]


def _rel_per_element(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    n = ref.shape[0]
    scale = np.abs(ref.reshape(n, -1)).max(axis=1)
    return (np.abs(got - ref).reshape(n, -1).max(axis=1) / scale).max()


@pytest.mark.parametrize("kind,name", FIXTURES)
def test_rest_tables_match_the_reference(kind, name):
    g = load_golden(name)
    s = pr.build_setup(kind, g["elements"], g["rest"])
    keys = {"edge_spring": ["d"], "tris_strain": ["P", "DmInv"], "tets_strain": ["DmInv"], "tets_deformation_gradient": ["DmInv"],
            "verts_bending": ["rest_curvature", "normal", "dot_with_normal"]}[kind]
    for k in keys:
        assert _rel_per_element(s.parts[k], g[k]) <= TABLE_TOL, k
    assert s.p == {"edge_spring": 1, "tris_strain": 2}.get(kind, 3 if kind.startswith("tets") else 1)
    assert s.rows == g["expected"].shape[1]
    assert s.table.shape[0] == s.n_elem * s.table_width + (0 if s.star_idx is None else s.star_idx.shape[0])


@pytest.mark.parametrize("name", ["cproj_verts_bending_grid", "cproj_verts_bending_closed"])
def test_bending_star_order_and_indices_are_the_reference_s(name):
    g = load_golden(name)
    s = pr.build_setup("verts_bending", g["elements"], g["rest"])
    assert s.bending_indices.tolist() == g["indices"].tolist()
    assert s.idx[:, 0].tolist() == g["indices"].tolist()
    assert s.star_ptr.tolist() == g["star_ptr"].tolist()
    assert s.star_idx.tolist() == g["star_idx"].tolist()
    # weights: per constrained vertex, against the largest weight of its star
    ptr = g["star_ptr"]
    for i in range(len(ptr) - 1):
        a, b = s.parts["weights"][ptr[i]:ptr[i + 1]], g["weights"][ptr[i]:ptr[i + 1]]
        assert np.abs(a - b).max() <= TABLE_TOL * np.abs(b).max()


def test_open_grid_skips_its_boundary_and_closed_mesh_keeps_every_vertex():
    g = load_golden("cproj_verts_bending_grid")
    tris, n = g["elements"], g["rest"].shape[0]
    # a boundary edge belongs to one triangle
    e = np.sort(np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]), axis=1)
    u, c = np.unique(e, axis=0, return_counts=True)
    boundary = set(u[c == 1].ravel().tolist())
    s = pr.build_setup("verts_bending", tris, g["rest"])
    assert s.bending_indices.tolist() == [v for v in range(n) if v not in boundary]
    g = load_golden("cproj_verts_bending_closed")
    s = pr.build_setup("verts_bending", g["elements"], g["rest"])
    assert s.bending_indices.tolist() == list(range(g["rest"].shape[0]))


@pytest.mark.parametrize("kind,name", FIXTURES + [("edge_spring", "cproj_edge_spring_collapsed")])
def test_host_restatement_reproduces_the_reference(kind, name):
    """``project_host`` (the scale leg of tools/time_cproj.py) on every fixture: 1e-12 absolute, the bound the device test
    uses on the raw tensor."""
    g = load_golden(name)
    s = pr.build_setup(kind, g["elements"], g["rest"])
    out = pr.project_host(s, g["frames"], *g["sigma"])
    assert out.shape == g["expected"].shape
    assert np.array_equal(np.isnan(out), np.isnan(g["expected"]))
    assert np.nanmax(np.abs(out - g["expected"])) <= 1e-12


# ------------------------------------------------------------------ refusals
def _snaps(F=3, tris=None):
    from fake_engine import FakeEngine
    from animsnapbases_amd import posSnapshots
    g = load_golden("cproj_tets_strain")
    with contextlib.redirect_stdout(io.StringIO()):
        return posSnapshots.from_arrays(g["frames"][:F], tris, "first", standarize=False, massWeight=False, engine=FakeEngine()), g


def test_refusals_name_their_cause():
    snaps, g = _snaps()
    N = g["rest"].shape[0]
    tets = g["elements"]
    with pytest.raises(ValueError, match="unknown projection kind"):
        snaps.constraint_projections("tets_stress", tets)
    with pytest.raises(ValueError, match=r"\(n, 4\) expected"):
        snaps.constraint_projections("tets_strain", tets[:, :3])
    with pytest.raises(ValueError, match=r"\(n, 2\) expected"):
        snaps.constraint_projections("edge_spring", tets)
    bad = tets.copy()
    bad[5, 2] = N
    with pytest.raises(ValueError, match="names vertex %d" % N):
        snaps.constraint_projections("tets_deformation_gradient", bad)
    bad[5, 2] = -1
    with pytest.raises(ValueError, match="names vertex -1"):
        snaps.constraint_projections("tets_strain", bad)
    flat = tets.copy()
    flat[7, 3] = flat[7, 0]                       # two equal corners: det Dm is exactly 0
    with pytest.raises(ValueError, match="degenerate rest element 7"):
        snaps.constraint_projections("tets_strain", flat)
    with pytest.raises(ValueError, match="degenerate rest element 0"):
        snaps.constraint_projections("edge_spring", np.array([[4, 4], [0, 1]]))
    with pytest.raises(ValueError, match="degenerate rest element 1"):
        snaps.constraint_projections("tris_strain", np.array([[0, 1, 3], [2, 2, 5]]))
    with pytest.raises(ValueError, match="sigma_min"):
        snaps.constraint_projections("tets_strain", tets, sigma_min=1.1, sigma_max=0.9)
    for rng in (dict(frame_start=2, frame_end=2), dict(frame_start=3), dict(frame_end=4), dict(frame_jump=0)):
        with pytest.raises(ValueError, match="empty frame range"):
            snaps.constraint_projections("tets_strain", tets, **rng)
    with pytest.raises(ValueError, match="no elements"):
        snaps.constraint_projections("verts_bending")         # no triangles on the snapshots
    with pytest.raises(ValueError, match="no test animation"):
        snaps.constraint_projections("tets_strain", tets, animation="test")
    with pytest.raises(ValueError, match="rest positions of shape"):
        snaps.constraint_projections("tets_strain", tets, rest_positions=g["rest"][:-1])


def test_several_ranks_are_refused():
    snaps, g = _snaps()
    snaps._comm = types.SimpleNamespace(multi=True)
    with pytest.raises(NotImplementedError, match="several ranks"):
        snaps.constraint_projections("tets_strain", g["elements"])
