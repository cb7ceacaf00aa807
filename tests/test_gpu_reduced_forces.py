"""GPU (-m gpu): the DEIM-reduced constraint forces b~ = S^T V (P^T V)^+ P^T p of a resident animation
(posSnapshots.reduced_constraint_forces / reduced_force_errors; asb_rforce_operator, asb_rforce_solver, asb_rforce_run and
asb_force_diff of csrc/asb_rforce.hip) against the fixtures the UNMODIFIED reference simulator wrote
(tools/gen_reduced_forces_golden.py: prepare_reduced_group, prepare_reduced_verts_bending, get_group_reduced_term, wi = 0.7).

Shapes.  k_rforce_gemm's tile is 64 frames (16 per wave) x 32 vertices, its contraction runs in steps of 4, k_cproj_em's tile is
16 elements x 64 frames: frame counts F' in {1, 17, 65, 130}, m in {1, 6, 17} (mp = 1 and 17 are padded to 4 and 20), a range
with frame_jump 3 and a start inside a tile, a held-out array; N = 18 (tetrahedra, closed bending mesh: one partial vertex
tile), 42 (triangle grid: two tiles), 135 (box: five tiles, the last partial, past the 128 rows of an MFMA block tile).

Bound of b~ against ``b_ref``: per coordinate d, derived in tests/reduced_forces_cases.py from the fixture alone,

    64 eps (kappa_d + mp + |Pt|) max_n sum_j |M_d[n, j]| max |coef_d|  +  tol_p || |M_d| |H_d| ||_inf

with tol_p = RAW_TOL = 1e-12 on the raw tensor and 64 eps max|x| / h kappa_F (tests/test_gpu_cproj.py) on the mass-weighted,
standardised one.  (M_d on the device is summed by FMA over ascending columns, in the bound's M_d by SciPy: nnz_n eps relative,
inside the first term's margin.)  Every measured error is printed beside its bound.

Error metrics: asb_force_diff's sums are sums of n non-negative terms in a fixed order, NumPy's of the same terms pairwise:
each within n eps of the exact sum, relatively; 4 n eps with the margin of 2 the project's other sums take.  The two maxima
are exact.  Bit-identity claims are checked with torch.equal."""
import contextlib
import io
import types

import numpy as np
import pytest

from reduced_forces_cases import CASES, COND_CAP, EPS, bound, case, operator, report
from test_gpu_cproj import _kappa, _min_edge

pytestmark = pytest.mark.gpu

ALL = [(name, m) for name in CASES for m in case(name).ms]


def _snaps(frames, standarize=False, mass=None, test_verts=None):
    from animsnapbases_amd import posSnapshots
    with contextlib.redirect_stdout(io.StringIO()):
        return posSnapshots.from_arrays(np.array(frames), None, "first", standarize=standarize, massWeight=mass is not None,
                                        mass=mass, test_verts=test_verts)


def _kw(c, **kw):
    return dict(dict(elements=c.g["elements"], wi=0.7, reduction=c.reduction, rest_positions=c.g["rest"],
                     sigma_min=c.g["sigma"][0], sigma_max=c.g["sigma"][1]), **kw)


# ------------------------------------------------------------------ 1. every fixture and m against the reference, raw tensor
@pytest.mark.parametrize("name,m", ALL)
def test_raw_tensor_matches_the_reference(name, m):
    c = case(name)
    F, N = c.g["frames"].shape[:2]
    op = operator(c, m)
    assert (op.cond <= COND_CAP).all()
    snaps = _snaps(c.g["frames"])
    out, nF = snaps.reduced_constraint_forces(c.kind, c.basis, m, **_kw(c))
    assert nF == F and tuple(out.shape) == (F, N, 3) and str(out.dtype) == "torch.float64" and out.is_cuda
    bnd = bound(c, m, op)
    err = report("%s m = %d (N = %d)" % (name, m, N), out.cpu().numpy(), c.r["b_ref_%d" % m], bnd)
    assert (err <= bnd).all()
    assert list(snaps.assembly_ST) == [c.kind] and snaps.assembly_ST[c.kind].shape == c.St.shape
    if c.kind == "verts_bending":
        assert snaps.bending_indices.tolist() == c.g["indices"].tolist()
    else:
        assert snaps.bending_indices is None


# ------------------------------------------------------------------ 2. frame counts and ranges around the tiles
@pytest.mark.parametrize("m", [1, 6, 17])
def test_frame_counts_and_ranges(m):
    c = case("tets_deim")
    op = operator(c, m)
    ref = c.r["b_ref_%d" % m]
    for F, f0, fj in ((1, 0, 1), (17, 0, 1), (65, 0, 1), (130, 0, 1), (130, 37, 3), (65, 63, 1)):
        sel = slice(f0, F, fj)
        snaps = _snaps(c.g["frames"][:F])
        out, nF = snaps.reduced_constraint_forces(c.kind, c.basis, m, frame_start=f0, frame_jump=fj, **_kw(c))
        assert nF == len(range(f0, F, fj)) and tuple(out.shape) == (nF, 18, 3)
        bnd = bound(c, m, op, frames=sel)
        err = report("m = %d F = %d start = %d jump = %d" % (m, F, f0, fj), out.cpu().numpy(), ref[sel], bnd)
        assert (err <= bnd).all(), (F, f0, fj)


# ------------------------------------------------------------------ 3. bit-identity
@pytest.mark.parametrize("name,m", [("tets_deim", 17), ("tris_blocks", 3), ("box", 5)])
@pytest.mark.parametrize("weighted", [False, True])
def test_repeats_ranges_and_accumulate_are_bit_identical(name, m, weighted):
    import torch
    from animsnapbases_amd import projections as proj
    c = case(name)
    F, N = c.g["frames"].shape[:2]
    mass = 0.5 + np.random.default_rng(4).random(N) if weighted else None
    snaps = _snaps(c.g["frames"], standarize=weighted, mass=mass)
    full = snaps.reduced_constraint_forces(c.kind, c.basis, m, **_kw(c))[0]
    assert torch.equal(snaps.reduced_constraint_forces(c.kind, c.basis, m, **_kw(c))[0], full)
    for f0, f1, fj in ((0, F, 3), (5, F, 1), (F // 2, F // 2 + 1, 1), (F // 2 + 1, F - 3, 3), (1, F, F - 2)):
        part, nF = snaps.reduced_constraint_forces(c.kind, c.basis, m, frame_start=f0, frame_end=f1, frame_jump=fj, **_kw(c))
        assert nF == len(range(f0, f1, fj))
        assert torch.equal(part, full[f0:f1:fj]), (f0, f1, fj)
    # through the engine: accumulate onto zeros gives the same bits; onto NaN nothing but NaN; accumulate = 0 overwrites NaN
    eng, op = snaps._engine, operator(c, m)
    setup = proj.build_setup(c.kind, c.g["elements"], c.g["rest"])
    eng.rforce_operator(proj.assembly_ST(setup, N, 0.7), op.V)
    eng.cproj_setup(proj.subset_setup(setup, op.elements))
    eng.rforce_solver(op.H, op.local_rows)
    args = (0, 0, F, 1, snaps.invMassL, weighted, snaps.pre_scale_factor, c.g["sigma"][0], c.g["sigma"][1])
    buf = torch.zeros_like(full)
    eng.rforce_run(*args, True, buf.data_ptr())
    assert torch.equal(buf, full)
    buf.fill_(float("nan"))
    eng.rforce_run(*args, False, buf.data_ptr())
    assert torch.equal(buf, full)
    eng.rforce_run(*args, True, buf.data_ptr())
    assert torch.equal(buf, full + full)


# ------------------------------------------------------------------ 4. held-out animation; mass-weighted, standardised tensor
def test_heldout_array():
    import torch
    c = case("tets_deim")
    m = 6
    full = _snaps(c.g["frames"]).reduced_constraint_forces(c.kind, c.basis, m, **_kw(c))[0]
    snaps = _snaps(c.g["frames"][:3])
    out, nF = snaps.reduced_constraint_forces(c.kind, c.basis, m, animation=np.array(c.g["frames"][10:]), frame_start=3,
                                              frame_jump=2, **_kw(c))
    sel = slice(13, None, 2)
    assert nF == len(range(13, 130, 2)) and torch.equal(out.cpu(), full[sel].cpu())        # (raw tensor: the same arithmetic)
    bnd = bound(c, m, operator(c, m), frames=sel)
    err = report("held-out m = %d" % m, out.cpu().numpy(), c.r["b_ref_%d" % m][sel], bnd)
    assert (err <= bnd).all()
    snaps = _snaps(c.g["frames"][:3], test_verts=np.array(c.g["frames"][10:]))
    out, nF = snaps.reduced_constraint_forces(c.kind, c.basis, m, animation="test", **_kw(c))
    assert nF == 120 and torch.equal(out.cpu(), full[10:].cpu())


@pytest.mark.parametrize("name,m", [("tets_deim", 6), ("tets_deim", 17), ("box", 10)])
def test_weighted_standardised_tensor(name, m):
    c = case(name)
    N = c.g["rest"].shape[0]
    g = dict(c.g)
    mass = 0.5 + np.random.default_rng(3).random(N)
    kap = _kappa(c.kind, g)
    tol_p = 64 * EPS * np.abs(g["frames"]).max() / _min_edge(c.kind, g) * kap
    op = operator(c, m)
    bnd = bound(c, m, op, tol_p=tol_p)
    snaps = _snaps(c.g["frames"], standarize=True, mass=mass)
    assert snaps.pre_scale_factor != 1 and snaps.massL is not None
    out, _ = snaps.reduced_constraint_forces(c.kind, c.basis, m, **_kw(c))
    err = report("%s m = %d weighted (kappa_F %.3g, tol_p %.3g)" % (name, m, kap, tol_p), out.cpu().numpy(), c.r["b_ref_%d" % m], bnd)
    assert (err <= bnd).all()
    # the same frames as a held-out animation of snapshots trained on the first three
    snaps = _snaps(c.g["frames"][:3], standarize=True, mass=mass)
    out, nF = snaps.reduced_constraint_forces(c.kind, c.basis, m, animation=np.array(c.g["frames"][2:]), frame_start=1, frame_jump=2,
                                              **_kw(c))
    sel = slice(3, None, 2)
    bnd = bound(c, m, op, tol_p=tol_p, frames=sel)
    err = report("%s m = %d weighted held-out" % (name, m), out.cpu().numpy(), c.r["b_ref_%d" % m][sel], bnd)
    assert nF == c.r["b_ref_%d" % m][sel].shape[0] and (err <= bnd).all()


# ------------------------------------------------------------------ 5. the error metrics
def _numpy_metrics(a, b):
    from animsnapbases_amd import constraintsComponents as cc
    rel = cc.relative_error_per_component(a, b)
    return cc.frobenius_error(a, b), cc.max_pointwise_error(a, b), rel[0], rel[1], rel[2]


@pytest.mark.parametrize("name", ["tets_deim", "box"])
def test_force_diff_against_numpy(name):
    c = case(name)
    m = c.ms[1]
    F, N = c.g["frames"].shape[:2]
    snaps = _snaps(c.g["frames"])
    full = snaps.constraint_forces([dict(kind=c.kind, elements=c.g["elements"], wi=0.7, rest_positions=c.g["rest"],
                                         sigma_min=c.g["sigma"][0], sigma_max=c.g["sigma"][1])])[0]
    red = snaps.reduced_constraint_forces(c.kind, c.basis, m, **_kw(c))[0]
    a, b = full.cpu().numpy(), red.cpu().numpy()
    sums, mx, norms, pf = snaps._engine.force_diff(full.data_ptr(), red.data_ptr(), F, N, per_frame=True)
    n = F * N
    e2, a2 = ((a - b) ** 2).sum(axis=(0, 1)), (a ** 2).sum(axis=(0, 1))
    print("%s sums rel err %s, norms rel err %s, allowed %.3g" % (name, np.abs(sums - e2) / e2, np.abs(norms[:3] - a2) / a2, 4 * n * EPS))
    assert (np.abs(sums - e2) <= 4 * n * EPS * e2).all() and (np.abs(norms[:3] - a2) <= 4 * n * EPS * a2).all()
    assert mx == np.abs(a - b).max() and norms[3] == a.max()
    ef, af = ((a - b) ** 2).sum(axis=(1, 2)), (a ** 2).sum(axis=(1, 2))
    assert pf.shape == (F, 2)
    assert (np.abs(pf[:, 0] - ef) <= 4 * 3 * N * EPS * ef).all() and (np.abs(pf[:, 1] - af) <= 4 * 3 * N * EPS * af).all()
    # the public method on the same run: the same device records, so the values of the formulas on them exactly ...
    got = snaps.reduced_force_errors(c.kind, c.basis, [m], per_frame=True, **_kw(c))
    assert got[0] == [float(np.sqrt(sums.sum()))] and got[1] == [mx / norms[3]]
    assert [got[2][0], got[3][0], got[4][0]] == [float(np.sqrt(sums[d]) / np.sqrt(norms[d])) for d in range(3)]
    assert got[5].shape == (1, F) and np.array_equal(got[5][0], np.sqrt(pf[:, 0]) / np.sqrt(pf[:, 1]))
    # ... and the reference's metrics of the downloaded pair within the sums' bound (a square root halves a relative error,
    # a quotient adds two)
    ref = _numpy_metrics(a, b)
    print("%s metrics %s" % (name, [g[0] for g in got[:5]]))
    print("%s numpy   %s" % (name, [float(v) for v in ref]))
    for i in range(5):
        assert abs(got[i][0] - ref[i]) <= 4 * n * EPS * abs(ref[i]), i
    assert list(snaps.assembly_ST) == [c.kind]


def test_a_sweep_equals_single_calls():
    c = case("tets_deim")
    snaps = _snaps(c.g["frames"])
    sweep = snaps.reduced_force_errors(c.kind, c.basis, [1, 6, 17], per_frame=True, **_kw(c))
    singles = [snaps.reduced_force_errors(c.kind, c.basis, [r], per_frame=True, **_kw(c)) for r in (1, 6, 17)]
    for i in range(5):
        assert sweep[i] == [s[i][0] for s in singles], i
    assert sweep[5].shape == (3, 130) and all(np.array_equal(sweep[5][j], singles[j][5][0]) for j in range(3))
    print("fro", sweep[0], "max", sweep[1])
    # an unsorted list: S^T V is built for the largest r wherever it stands
    back = snaps.reduced_force_errors(c.kind, c.basis, [17, 1], **_kw(c))
    assert [back[i][::-1] for i in range(5)] == [[sweep[i][0], sweep[i][2]] for i in range(5)]
    # held-out frames and a range
    part = snaps.reduced_force_errors(c.kind, c.basis, [6], animation=np.array(c.g["frames"][40:]), frame_start=5, frame_jump=3, **_kw(c))
    assert all(np.isfinite(v[0]) for v in part)


# ------------------------------------------------------------------ 6. end to end: positions -> projections -> POD -> DEIM -> force errors
def test_end_to_end_from_positions(tmp_path):
    from animsnapbases_amd import constraintsComponents, nonlinearSnapshots
    c = case("tets_deim")
    K = 12
    param = types.SimpleNamespace(constProj_rest_shape="first", constProj_numFrames=0, constProj_p_size=3,
                                  constProj_massWeight=False, constProj_standarize=False, constProj_orthogonal=False,
                                  constProj_basis_type="pod_vectorized", deim_desired_num_components=K,
                                  constProj_store_sing_val=False, constProj_output_directory=str(tmp_path), name="rf",
                                  constProj_name="tets", constProj_bases_interpolation_type="deim",
                                  constProj_snapshots_type="tets_strain")
    snaps = _snaps(c.g["frames"])
    kw = dict(rest_positions=c.g["rest"], sigma_min=c.g["sigma"][0], sigma_max=c.g["sigma"][1])
    with contextlib.redirect_stdout(io.StringIO()):
        ns = nonlinearSnapshots.from_positions(param, snaps, "tets_strain", c.g["elements"], wi=0.7, **kw)
        ns.config()
        ns.snapshots_prepare()
        cc = constraintsComponents(param, ns)
        cc.config()
        cc.compute_components_store_singvalues()
        cc.deim()
    assert cc.geom_Pt.shape == (K,)
    rs = list(range(1, K + 1))
    fro, mx, rx, ry, rz = snaps.reduced_force_errors("tets_strain", cc, rs, elements=c.g["elements"], wi=0.7,
                                                     reduction="deim_pod_vectorized", **kw)
    print("fro", fro)
    vals = np.array([fro, mx, rx, ry, rz])
    assert np.isfinite(vals).all() and (vals > 0).all()
    # the trend (a DEIM error need not fall at every step): the last below the first, the later half below the earlier on average
    assert fro[-1] < fro[0] and np.mean(fro[K // 2:]) < np.mean(fro[:K // 2])
    alone = snaps.reduced_force_errors("tets_strain", cc, [K], elements=c.g["elements"], wi=0.7, reduction="deim_pod_vectorized", **kw)
    assert [v[0] for v in alone] == [fro[-1], mx[-1], rx[-1], ry[-1], rz[-1]]
    # the stored file serves as the basis too: the same bits
    with contextlib.redirect_stdout(io.StringIO()):
        cc.store_components_n_interpol_points()
    path = tmp_path / "components_interpol_alphas_interpol_verts_interpol_alpha_ranges.npz"
    again = snaps.reduced_force_errors("tets_strain", str(path), [K], elements=c.g["elements"], wi=0.7,
                                       reduction="deim_pod_vectorized", **kw)
    assert again == alone


# ------------------------------------------------------------------ 7. the C entries refuse what does not fit
def test_the_c_entries_check_their_arguments():
    import torch
    from animsnapbases_amd import projections as proj
    c = case("tets_deim")
    N = 18
    snaps = _snaps(c.g["frames"][:3])
    eng, op = snaps._engine, operator(c, 6)
    setup = proj.build_setup(c.kind, c.g["elements"], c.g["rest"])
    St = proj.assembly_ST(setup, N, 0.7)
    out = torch.zeros((3, N, 3), dtype=torch.float64, device="cuda:%d" % eng.device_id)
    args = (0, 0, 3, 1, None, False, 1.0, 1.0, 1.0, False, out.data_ptr())
    eng.cproj_setup(proj.subset_setup(setup, op.elements))
    with pytest.raises(RuntimeError, match="no operator"):
        eng.rforce_solver(op.H, op.local_rows)
    with pytest.raises(RuntimeError, match="rows"):
        eng.rforce_operator(St[:N - 1], op.V)
    with pytest.raises(RuntimeError, match="names column"):
        eng.rforce_operator(St, np.ascontiguousarray(op.V[:-3]))
    with pytest.raises(RuntimeError, match="no operator or solver"):
        eng.rforce_run(*args)
    eng.rforce_operator(St, op.V)
    with pytest.raises(RuntimeError, match="no operator or solver"):            # (a new operator drops the solver)
        eng.rforce_run(*args)
    with pytest.raises(RuntimeError, match="7 basis vectors, the operator has 6"):
        eng.rforce_solver(np.zeros((3, 7, 6)), op.local_rows)
    rows = op.local_rows.copy()
    rows[2] = op.elements.shape[0] * 3
    eng.rforce_solver(op.H, rows)
    with pytest.raises(RuntimeError, match="names row 18, the sampled elements have 18"):
        eng.rforce_run(*args)
    with pytest.raises(RuntimeError, match="not a selection"):
        eng.rforce_run(0, 0, 4, 1, *args[4:])
    assert (out == 0).all().item()
    eng.rforce_solver(op.H, op.local_rows)
    eng.rforce_run(*args)
    assert (out != 0).any().item()
    with pytest.raises(RuntimeError, match="0 frames"):
        eng.force_diff(out.data_ptr(), out.data_ptr(), 0, N)
    sums, mx, norms, pf = eng.force_diff(out.data_ptr(), out.data_ptr(), 3, N)
    assert (sums == 0).all() and mx == 0 and pf is None and norms[3] == out.max().item()
