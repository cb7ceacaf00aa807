"""CPU: the host restatement of the reference's reduced operator (animsnapbases_amd/reduced.py) against the fixtures the
UNMODIFIED reference simulator wrote (tools/gen_reduced_forces_golden.py: prepare_reduced_group,
prepare_reduced_verts_bending, get_group_reduced_term), its refusals, and the refusals of the public methods that need no
device (through the CPU engine double).

  * the sampled elements, the rows Pt and the Tikhonov terms la are EQUAL to the reference's;
  * S^T V_d (sparse) against the reference's dense einsum ``projecting_mat``: entry (n, j) within nnz_n eps sum_c |S_nc| |V_cj|
    (a sum of nnz_n non-zero products, in either order);
  * (S^T V_d) (H_d p[Pt]) against ``b_ref`` within the bound of tests/reduced_forces_cases.py, with the reference's own p.
The condition numbers are recomputed and held to the fixtures' cap of 1e6 (a condition on the fixture, not a tolerance)."""
import contextlib
import io
import types

import numpy as np
import pytest

from reduced_forces_cases import CASES, COND_CAP, EPS, bound, case, operator, report

ALL = [(name, m) for name in CASES for m in case(name).ms]


@pytest.mark.parametrize("name,m", ALL)
def test_operator_equals_the_reference(name, m):
    c = case(name)
    op = operator(c, m)
    assert op.Pt.tolist() == c.r["Pt_%d" % m].tolist()
    assert op.elements.tolist() == c.r["alphas_%d" % m].tolist()
    assert np.array_equal(op.la, c.r["la_%d" % m])
    mp = m * op.row_dim
    assert op.V.shape == (c.r["components"].shape[1], mp, 3) and op.H.shape == (3, mp, op.Pt.shape[0])
    assert op.local_rows.shape == op.Pt.shape and op.local_rows.max() < op.elements.shape[0] * c.p
    # the sampled rows in the stack of the sampled elements alone are the rows Pt of the full stack
    assert (op.elements[op.local_rows // c.p] * c.p + op.local_rows % c.p).tolist() == op.Pt.tolist()
    print("%s m = %d: cond %s (stored %s)" % (name, m, op.cond, c.r["cond_%d" % m]))
    assert (op.cond <= COND_CAP).all() and (c.r["cond_%d" % m] <= COND_CAP).all()
    assert np.allclose(op.cond, c.r["cond_%d" % m], rtol=1e-6)


@pytest.mark.parametrize("name", list(CASES))
def test_sparse_st_v_against_the_dense_einsum(name):
    c = case(name)
    m = c.ms[-1]
    op = operator(c, m)
    pm = c.r["projecting_mat_%d" % m]
    nnz = np.diff(c.St.indptr).astype(np.float64)[:, None]
    A = abs(c.St)
    for d in range(3):
        got = c.St @ op.V[:, :, d]
        tol = nnz * EPS * (A @ np.abs(op.V[:, :, d]))
        err = np.abs(got - pm[:, :, d])
        print("%s d = %d: max err %.3g, largest err / tol %.3g" % (name, d, err.max(), (err / np.where(tol > 0, tol, 1)).max()))
        assert (err <= tol).all()


@pytest.mark.parametrize("name,m", ALL)
def test_reduced_term_against_the_reference(name, m):
    c = case(name)
    op = operator(c, m)
    P = c.p_pt(m)
    got = np.empty(c.r["b_ref_%d" % m].shape)
    for d in range(3):
        got[:, :, d] = ((c.St @ op.V[:, :, d]) @ (op.H[d] @ P[:, :, d].T)).T
    bnd = bound(c, m, op)
    err = report("%s m = %d" % (name, m), got, c.r["b_ref_%d" % m], bnd)
    assert (err <= bnd).all()


def test_subset_setup_takes_the_tables_over():
    from animsnapbases_amd import projections as proj
    for name in ("tets_deim", "bending"):
        c = case(name)
        full = proj.build_setup(c.kind, c.g["elements"], c.g["rest"])
        sel = np.array([5, 0, 5, full.n_elem - 1])
        sub = proj.subset_setup(full, sel)
        assert sub.n_elem == 4 and sub.rows == 4 * c.p
        a = proj.project_host(full, c.g["frames"][:5], *c.g["sigma"]) if name != "bending" else None
        if a is not None:                                   # (the NumPy projection: same tables, same values)
            sub.parts = {k: v[sel] for k, v in full.parts.items()}
            b = proj.project_host(sub, c.g["frames"][:5], *c.g["sigma"])
            rows = (sel[:, None] * c.p + np.arange(c.p)[None]).reshape(-1)
            assert np.array_equal(b, a[:, rows])
        else:
            assert sub.bending_indices.tolist() == full.bending_indices[sel].tolist()
            deg = np.diff(full.star_ptr)[sel]
            assert np.diff(sub.star_ptr).tolist() == deg.tolist() and sub.star_idx.shape[0] == deg.sum()
            assert sub.table.shape[0] == 4 * 5 + deg.sum()
            i0 = full.star_ptr[5]
            assert np.array_equal(sub.star_idx[:deg[0]], full.star_idx[i0:i0 + deg[0]])
    with pytest.raises(ValueError, match="elements 0.."):
        proj.subset_setup(full, [full.n_elem])


# ------------------------------------------------------------------ refusals of the host operator
def test_operator_refusals():
    from animsnapbases_amd import reduced
    c = case("tets_deim")
    b = c.basis
    K, rows = b["components"].shape[:2]
    args = lambda **kw: dict(dict(components=b["components"], interpol_alphas=b["interpol_alphas"], Pt=b["Pt"],
                                  interpol_alpha_ranges=b["interpol_alpha_ranges"], num_components=6, p=3,
                                  reduction="deim_pod_vectorized"), **kw)
    with pytest.raises(ValueError, match="unknown reduction"):
        reduced.reduced_operator(**args(reduction="deim"))
    for m in (0, K + 1):
        with pytest.raises(ValueError, match=r"outside 1\.\.%d" % K):
            reduced.reduced_operator(**args(num_components=m))
    with pytest.raises(ValueError, match=r"outside 1\.\.%d" % (K // 3)):           # blocks: m p vectors are needed
        reduced.reduced_operator(**args(num_components=K // 3 + 1, reduction="deim_pca_blocks"))
    with pytest.raises(ValueError, match="exist for r <= 4 only"):
        reduced.reduced_operator(**args(interpol_alpha_ranges=b["interpol_alpha_ranges"][:4]))
    with pytest.raises(ValueError, match="no interpolation points"):
        reduced.reduced_operator(**args(interpol_alpha_ranges=np.zeros(0, dtype=np.int64)))
    with pytest.raises(ValueError, match="5 interpolation rows for 6 basis vectors"):
        reduced.reduced_operator(**args(interpol_alpha_ranges=np.minimum(b["interpol_alpha_ranges"], 5)))
    with pytest.raises(ValueError, match="2 interpolation rows for 6 basis vectors"):      # blocks of p = 2: one element, three blocks
        reduced.reduced_operator(**args(num_components=3, p=2, reduction="geom_pca_blocks_withSt",
                                        interpol_alpha_ranges=np.array([1, 1, 1])))
    Pt = b["Pt"].copy()
    Pt[2] = rows
    with pytest.raises(ValueError, match="names row %d" % rows):
        reduced.reduced_operator(**args(Pt=Pt))
    al = b["interpol_alphas"].copy()
    al[1] = -1
    with pytest.raises(ValueError, match="names element -1"):
        reduced.reduced_operator(**args(interpol_alphas=al))
    al[1] = rows // 3
    with pytest.raises(ValueError, match="names element %d" % (rows // 3)):
        reduced.reduced_operator(**args(interpol_alphas=al, reduction="deim_pca_blocks", num_components=2))
    with pytest.raises(ValueError, match="%d rows, %d elements x 3 expected" % (rows, rows // 3 + 1)):
        reduced.reduced_operator(**args(n_elements=rows // 3 + 1))
    with pytest.raises(ValueError, match="elements x 2 expected"):
        reduced.reduced_operator(**args(components=b["components"][:, :rows - 1], p=2))
    with pytest.raises(ValueError, match=r"\(K, rows, 3\) expected"):
        reduced.reduced_operator(**args(components=b["components"][:, :, :2]))


def test_load_basis_takes_three_forms(tmp_path):
    from animsnapbases_amd import reduced
    c = case("bending")
    path = tmp_path / "components_interpol_alphas_interpol_verts_interpol_alpha_ranges.npz"
    np.savez(path, interpol_verts=np.zeros(0), **c.basis)
    cc = types.SimpleNamespace(comps=c.basis["components"], geom_alpha=c.basis["interpol_alphas"], geom_Pt=c.basis["Pt"],
                               geom_alpha_ranges=c.basis["interpol_alpha_ranges"])
    for form in (str(path), path, dict(c.basis), cc):
        d = reduced.load_basis(form)
        assert sorted(d) == sorted(reduced.BASIS_KEYS)
        for k in reduced.BASIS_KEYS:
            assert np.array_equal(d[k], c.basis[k])
    with pytest.raises(ValueError, match="no 'Pt'"):
        reduced.load_basis({k: v for k, v in c.basis.items() if k != "Pt"})
    cc.geom_alpha_ranges = None
    with pytest.raises(ValueError, match="no interpolation points"):
        reduced.load_basis(cc)


# ------------------------------------------------------------------ refusals of the public methods (no device needed)
def _snaps(F=3):
    from fake_engine import FakeEngine
    from animsnapbases_amd import posSnapshots
    c = case("tets_deim")
    with contextlib.redirect_stdout(io.StringIO()):
        return posSnapshots.from_arrays(np.array(c.g["frames"][:F]), None, "first", standarize=False, massWeight=False,
                                        engine=FakeEngine()), c


def _kw(c, **kw):
    return dict(dict(elements=c.g["elements"], wi=0.7, reduction=c.reduction, rest_positions=c.g["rest"],
                     sigma_min=c.g["sigma"][0], sigma_max=c.g["sigma"][1]), **kw)


def test_public_methods_refuse_before_the_device():
    snaps, c = _snaps()
    for call in (lambda **kw: snaps.reduced_constraint_forces(kw.pop("kind", c.kind), kw.pop("basis", c.basis), kw.pop("m", 6), **_kw(c, **kw)),
                 lambda **kw: snaps.reduced_force_errors(kw.pop("kind", c.kind), kw.pop("basis", c.basis), [kw.pop("m", 6)], **_kw(c, **kw))):
        with pytest.raises(ValueError, match="unknown projection kind"):
            call(kind="tets_stress")
        with pytest.raises(ValueError, match="sigma_min"):
            call(sigma_min=1.1, sigma_max=0.9)
        with pytest.raises(ValueError, match="empty frame range"):
            call(frame_start=3)
        with pytest.raises(ValueError, match="no test animation"):
            call(animation="test")
        with pytest.raises(ValueError, match="unknown reduction"):
            call(reduction="pod")
        with pytest.raises(ValueError, match="finite"):
            call(wi=float("nan"))
        with pytest.raises(ValueError, match=r"outside 1\.\.20"):
            call(m=21)
        with pytest.raises(ValueError, match="elements x 3 expected"):
            call(elements=c.g["elements"][:-1])
        with pytest.raises(ValueError, match="no 'components'"):
            call(basis={})
    assert snaps.assembly_ST is None and snaps.bending_indices is None
    assert snaps.reduced_force_errors(c.kind, c.basis, [], **_kw(c)) == ([], [], [], [], [])


def test_several_ranks_are_refused():
    snaps, c = _snaps()
    snaps._comm = types.SimpleNamespace(multi=True)
    with pytest.raises(NotImplementedError, match="several ranks"):
        snaps.reduced_constraint_forces(c.kind, c.basis, 6, **_kw(c))
    with pytest.raises(NotImplementedError, match="several ranks"):
        snaps.reduced_force_errors(c.kind, c.basis, [1, 6], **_kw(c))
