"""GPU (-m gpu): the constraint forces b[f] = sum_k S_k^T p_k(q_f) of a resident animation (posSnapshots.constraint_forces,
asb_cforce_run; k_cproj_em / k_st_apply of csrc/asb_cproj.hip) and the S^T that from_positions(wi=...) leaves for the
constraint bases, against fixtures written by the UNMODIFIED reference classes with wi = 0.7 (tools/gen_golden_st.py:
the reference's ``*_assembly_ST`` and ``assembly_ST @ stacked_p`` per frame, Simulators.py:643-724).

Shapes.  k_cproj_em's tile is 16 elements x 64 frames, k_st_apply's 16 vertices x 64 frames, chunks are multiples of 16 frames:
element subsets e in {1, 17, 68} (most vertices then have EMPTY rows of S^T), frame counts F in {1, 17, 65, 130}, a range
with frame_jump 3 and a start inside a tile, chunk_frames = 16 on 130 frames (nine chunks, the last one partial).  The meshes
have 18 (tets, edges), 42 (grid) vertices: two and three vertex blocks, the last one partial.

Tolerance of one entry b[f, v, d] = sum_j S_vj p_j[f, d], from the fixture alone:

    |b_dev - b_ref| <= tol_p * sum_j |S_vj|  +  4 nnz_v eps sum_j |S_vj| ||p_j||_inf

  * first term: the device's p_j differs from the reference's by at most tol_p entrywise -- RAW_TOL = 1e-12 on the raw tensor,
    64 eps (max|x| / min rest edge) kappa on the mass-weighted, standardised one, both the figures (and the derivations) of
    tests/test_gpu_cproj.py -- and the sum passes that on with the weights |S_vj|.  (The device's S_vj differs from the
    reference's by 1e-13 relative at most, tests/test_st_assembly_cpu.py: below the second term.)
  * second term: an n-term sum of products in floating point, in any order, with or without FMA, is within
    n eps sum |S_vj| |p_j| of the exact sum (gamma_n <= n eps (1 + n eps), n = nnz_v <= 40 here).  Device (FMA, ascending
    columns) and reference (SciPy's CSR product) each commit one such error: 2 n eps; the margin of 2 gives 4 n eps.
    ||p_j||_inf: the largest |p_j[f, d]| over the fixture's frames.
Two kinds in one call: the sum of both kinds' bounds (plus eps |b| for the one addition of the two terms, inside the margin).
Bit-identity claims (repeats, sub-ranges, chunk widths) are checked with torch.equal."""
import contextlib
import io
import types

import numpy as np
import pytest
from scipy import sparse

from conftest import load_golden
from test_gpu_cproj import RAW_TOL, _kappa, _min_edge

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
KINDS = ["edge_spring", "tris_strain", "tets_strain", "tets_deformation_gradient"]
ALL = KINDS + ["verts_bending_grid", "verts_bending_closed"]
_cache = {}


def _g(name):
    """(cproj fixture, st fixture, the reference's S^T as CSR); read once, read-only."""
    if name not in _cache:
        g = load_golden("cproj_" + name)
        s = load_golden("st_" + name)
        for v in list(g.values()) + list(s.values()):
            v.setflags(write=False)
        St = sparse.coo_matrix((s["val"], (s["row"], s["col"])), shape=tuple(s["shape"])).tocsr()
        assert float(s["wi"]) == 0.7
        _cache[name] = (g, s, St)
    return _cache[name]


def _kind(name):
    return "verts_bending" if name.startswith("verts_bending") else name.replace("_collapsed", "")


def _snaps(frames, standarize=False, mass=None, test_verts=None):
    from animsnapbases_amd import posSnapshots
    with contextlib.redirect_stdout(io.StringIO()):
        return posSnapshots.from_arrays(np.array(frames), None, "first", standarize=standarize, massWeight=mass is not None,
                                        mass=mass, test_verts=test_verts)


def _spec(name, e=None, **kw):
    g = _g(name)[0]
    d = dict(kind=_kind(name), elements=g["elements"] if e is None else g["elements"][:e], wi=0.7, rest_positions=g["rest"],
             sigma_min=g["sigma"][0], sigma_max=g["sigma"][1])
    d.update(kw)
    return d


def _bound(St, p, tol_p):
    """(N, 1) bound on |b_dev - b_ref| (module docstring) for the reference's S^T (N, rows) and projections p (F, rows, 3)."""
    A = abs(St).tocsr()
    nnz = np.diff(A.indptr).astype(np.float64)
    pinf = np.abs(p).max(axis=(0, 2)) if p.shape[0] else np.zeros(p.shape[1])
    return (tol_p * np.asarray(A.sum(axis=1)).ravel() + 4.0 * nnz * EPS * (A @ pinf))[:, None]


def _report(tag, got, ref, bound):
    err = np.abs(got - ref)
    worst = (err / np.where(bound > 0, bound, 1.0)).max()
    print("%s: max abs err %.3g, largest err / bound %.3g (smallest non-zero bound %.3g)"
          % (tag, err.max(), worst, bound[bound > 0].min()))
    return err


# ------------------------------------------------------------------ 1. every kind against the golden b, raw tensor
@pytest.mark.parametrize("name", ALL)
def test_raw_tensor_matches_the_reference(name):
    g, s, St = _g(name)
    F, N = g["frames"].shape[:2]
    snaps = _snaps(g["frames"])
    out, nF = snaps.constraint_forces([_spec(name)])
    assert nF == F and tuple(out.shape) == (F, N, 3) and str(out.dtype) == "torch.float64" and out.is_cuda
    bound = _bound(St, g["expected"], RAW_TOL)
    err = _report(name, out.cpu().numpy(), s["b"], bound)
    assert (err <= bound[None]).all()
    mine = snaps.assembly_ST[_kind(name)]
    assert list(snaps.assembly_ST) == [_kind(name)] and mine.shape == St.shape and mine.has_sorted_indices
    if name.startswith("verts_bending"):
        assert snaps.bending_indices.tolist() == g["indices"].tolist()
    else:
        assert snaps.bending_indices is None


# ------------------------------------------------------------------ 2. shapes around the tiles; empty rows are exactly 0.0
@pytest.mark.parametrize("name", KINDS)
def test_shapes_around_the_tiles(name):
    import torch
    from animsnapbases_amd import projections as proj
    g, s, St = _g(name)
    N = g["rest"].shape[0]
    p = St.shape[1] // g["elements"].shape[0]
    cases = [(1, 1, 0, 1, None), (17, 17, 0, 1, None), (68, 65, 0, 1, None), (1, 130, 0, 1, None), (17, 130, 0, 1, 16),
             (68, 130, 0, 1, 16), (68, 130, 37, 3, None), (1, 130, 70, 3, 16)]
    for e, F, f0, fj, chunk in cases:
        sub = St[:, :e * p]                                         # column block e of the assembly is element e's alone
        sel = range(f0, F, fj)
        pe = g["expected"][f0:F:fj, :e * p]
        ref = np.stack([sub @ pe[i] for i in range(len(sel))])
        snaps = _snaps(g["frames"][:F])
        out, nF = snaps.constraint_forces([_spec(name, e)], frame_start=f0, frame_jump=fj, chunk_frames=chunk)
        assert nF == len(sel) and tuple(out.shape) == (len(sel), N, 3)
        got = out.cpu().numpy()
        bound = _bound(sub, pe, RAW_TOL)
        err = _report("%s e=%d F=%d start=%d jump=%d chunk=%s" % (name, e, F, f0, fj, chunk), got, ref, bound)
        assert (err <= bound[None]).all(), (e, F, f0, fj, chunk)
        empty = np.diff(sub.indptr) == 0
        assert empty.sum() >= (N - 4 if e == 1 else 0)
        # the same call through the engine into a buffer full of NaN: accumulate = 0 writes EVERY entry
        setup = proj.build_setup(name, g["elements"][:e], g["rest"])
        buf = torch.full((len(sel), N, 3), float("nan"), dtype=torch.float64, device=out.device)
        eng = snaps._engine
        eng.cproj_setup(setup)
        eng.cforce_run(0, f0, F, fj, None, False, 1.0, g["sigma"][0], g["sigma"][1], proj.assembly_ST(setup, N, 0.7), False,
                       chunk or 0, buf.data_ptr())
        assert torch.equal(buf, out), (e, F, f0, fj, chunk)
        z = buf.cpu().numpy()[:, empty]
        assert (z == 0.0).all() and not np.signbit(z).any(), (e, F)


# ------------------------------------------------------------------ 3. bit-identity
@pytest.mark.parametrize("name", ["tets_strain", "edge_spring", "verts_bending_grid"])
@pytest.mark.parametrize("weighted", [False, True])
def test_repeats_ranges_and_chunks_are_bit_identical(name, weighted):
    import torch
    g = _g(name)[0]
    F = g["frames"].shape[0]
    mass = 0.5 + np.random.default_rng(4).random(g["rest"].shape[0]) if weighted else None
    snaps = _snaps(g["frames"], standarize=weighted, mass=mass)
    spec = [_spec(name)]
    full = snaps.constraint_forces(spec)[0]
    assert torch.equal(snaps.constraint_forces(spec)[0], full)
    for chunk in (16, 17, 64):                                      # 17 rounds up to 32
        assert torch.equal(snaps.constraint_forces(spec, chunk_frames=chunk)[0], full), chunk
    for f0, f1, fj, chunk in ((0, F, 3, None), (5, F, 1, 16), (37, 38, 1, None), (63, 66, 1, 16), (F // 2 + 5, F - 3, 3, None),
                              (1, 66, 64, None)):
        part, nF = snaps.constraint_forces(spec, frame_start=f0, frame_end=f1, frame_jump=fj, chunk_frames=chunk)
        assert nF == len(range(f0, f1, fj))
        assert torch.equal(part, full[f0:f1:fj]), (f0, f1, fj, chunk)


# ------------------------------------------------------------------ 4. two kinds in one call
def test_two_kinds_add_in_list_order():
    import torch
    ge, _, St_e = _g("edge_spring")
    gt, _, St_t = _g("tets_strain")
    c = load_golden("st_combined")
    fr = gt["frames"]
    assert (np.linalg.norm(fr[:, ge["elements"][:, 0]] - fr[:, ge["elements"][:, 1]], axis=2) > 0).all()
    snaps = _snaps(fr)
    edge, tet = _spec("edge_spring"), _spec("tets_strain")
    out, nF = snaps.constraint_forces([edge, tet])
    assert nF == fr.shape[0] and list(snaps.assembly_ST) == ["edge_spring", "tets_strain"]
    bound = _bound(St_e, c["p_edge"], RAW_TOL) + _bound(St_t, gt["expected"], RAW_TOL)
    err = _report("edge + tets", out.cpu().numpy(), c["b"], bound)
    assert (err <= bound[None]).all()
    # each term alone, added by torch in the same order: the same bits (one thread, kinds in list order)
    only_e = snaps.constraint_forces([edge])[0]
    only_t = snaps.constraint_forces([tet])[0]
    assert torch.equal(only_e + only_t, out)
    assert torch.equal(snaps.constraint_forces([edge, tet], chunk_frames=16)[0], out)
    # the order is the caller's: the reversed list agrees within the bound (and is the other sum of the same two terms)
    rev = snaps.constraint_forces([tet, edge])[0]
    assert list(snaps.assembly_ST) == ["tets_strain", "edge_spring"]
    err = _report("tets + edge", rev.cpu().numpy(), c["b"], bound)
    assert (err <= bound[None]).all()
    assert torch.equal(only_t + only_e, rev)


# ------------------------------------------------------------------ 5. mass-weighted, standardised tensor; held-out animation
@pytest.mark.parametrize("name", KINDS + ["verts_bending_grid"])
def test_weighted_standardised_tensor_and_heldout(name):
    g, s, St = _g(name)
    kind = _kind(name)
    N = g["rest"].shape[0]
    mass = 0.5 + np.random.default_rng(3).random(N)
    kap = _kappa(kind, g)
    tol_p = 64 * EPS * np.abs(g["frames"]).max() / _min_edge(kind, g) * kap
    bound = _bound(St, g["expected"], tol_p)
    snaps = _snaps(g["frames"], standarize=True, mass=mass)
    assert snaps.pre_scale_factor != 1 and snaps.massL is not None
    out, _ = snaps.constraint_forces([_spec(name)])
    err = _report("%s (kappa %.3g, tol_p %.3g) train" % (name, kap, tol_p), out.cpu().numpy(), s["b"], bound)
    assert (err <= bound[None]).all()
    # the same frames as a held-out animation of snapshots trained on the first three: weighted and scaled the same way
    snaps = _snaps(g["frames"][:3], standarize=True, mass=mass)
    out, nF = snaps.constraint_forces([_spec(name)], animation=np.array(g["frames"][10:]), frame_start=3, frame_jump=2,
                                      chunk_frames=16)
    ref = s["b"][13::2]
    assert nF == ref.shape[0]
    err = _report("%s held-out" % name, out.cpu().numpy(), ref, bound)
    assert (err <= bound[None]).all()


def test_heldout_raw_equals_the_train_run():
    import torch
    g = _g("tets_strain")[0]
    full = _snaps(g["frames"]).constraint_forces([_spec("tets_strain")])[0]
    snaps = _snaps(g["frames"][:3], test_verts=np.array(g["frames"][10:]))
    out, nF = snaps.constraint_forces([_spec("tets_strain")], animation="test")
    assert nF == g["frames"].shape[0] - 10 and torch.equal(out.cpu(), full[10:].cpu())


# ------------------------------------------------------------------ 6. collapsed edge
def test_collapsed_edge_reaches_exactly_its_two_vertices():
    g, s, St = _g("edge_spring_collapsed")
    nan_ref = np.isnan(s["b"])
    assert nan_ref.any(axis=2).sum() == 2 and sorted(np.flatnonzero(nan_ref[2].any(axis=1)).tolist()) == sorted(g["elements"][3].tolist())
    snaps = _snaps(g["frames"])
    out = snaps.constraint_forces([_spec("edge_spring_collapsed")])[0].cpu().numpy()
    assert np.array_equal(np.isnan(out), nan_ref)
    assert np.isfinite(out[~nan_ref]).all()
    bound = np.broadcast_to(_bound(St, np.nan_to_num(g["expected"]), RAW_TOL)[None], out.shape)
    assert (np.abs(out - s["b"])[~nan_ref] <= bound[~nan_ref]).all()


# ------------------------------------------------------------------ 7. end to end: S^T bases without an S^T file
def _st_param(tmp):
    return types.SimpleNamespace(constProj_rest_shape="first", constProj_numFrames=0, constProj_p_size=3,
                                 constProj_massWeight=False, constProj_standarize=True, constProj_orthogonal=False,
                                 constProj_basis_type="pca_blocks_with_St", deim_desired_num_components=0,
                                 constProj_store_sing_val=False, constProj_support="global", constProj_output_directory=str(tmp),
                                 name="st", constProj_name="tets", constProj_bases_interpolation_type="geom",
                                 constProj_snapshots_type="tets_strain", constProj_element_type="_tets", bases_R_tol=3.0,
                                 geom_ele_per_vert=2)


def _st_run(g, tmp, St=None, watch=None):
    from animsnapbases_amd import constraintsComponents, nonlinearSnapshots
    param = _st_param(tmp)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        snaps = _snaps(g["frames"])
        ns = nonlinearSnapshots.from_positions(param, snaps, "tets_strain", g["elements"], wi=0.7, rest_positions=g["rest"],
                                               sigma_min=g["sigma"][0], sigma_max=g["sigma"][1])
        ns.config()
        ns.tets = g["elements"]
        ns.snapshots_prepare()
        cc = constraintsComponents(param, ns)
        cc.config()
        assert cc.St is ns.assembly_ST and cc.St is snaps.assembly_ST["tets_strain"]       # no S^T file: the assembled one
        if St is not None:
            cc.St = St
        if watch is not None:
            watch(ns, cc)
        cc.compute_components_store_singvalues()
    verts = [int(ln.split()[1]) for ln in buf.getvalue().splitlines() if ln.startswith("vert ")]
    return verts, cc


def test_end_to_end_st_bases_without_an_st_file(tmp_path):
    """from_positions("tets_strain", wi=0.7) -> 'pca_blocks_with_St' with the assembled S^T, against the same run with ``St``
    assigned from the reference's matrix: the same vertex sequence; rank-1 terms within 1e-6 and weights within 1e-9, the
    tolerances tests/test_gpu_blocks_deim.py holds this path to.  bases_R_tol = 3.0 is about 1 % of |R| = 283 of the
    standardised tensor: a handful of vertices, some hundred components.  The first (up to three) picks are checked to be no near-ties
    (a second-largest row energy of S^T R within 1e-6 of the largest could swap under the 1e-13 difference of the two S^T)."""
    g, _, St_ref = _g("tets_strain")
    gaps = []

    def watch(ns, cc):
        eng, inner = ns._engine, ns._engine.st_residual_argmax

        def argmax():
            v, val = inner()
            if len(gaps) < 3:
                R = eng.download_residual()
                E = np.sort(sum(((cc.St @ R[f]) ** 2).sum(axis=1) for f in range(R.shape[0])))
                gaps.append((E[-1] - E[-2]) / E[-1])
            return v, val
        eng.st_residual_argmax = argmax

    vA, ccA = _st_run(g, tmp_path, watch=watch)
    print("vertices", vA, "relative gaps of the first picks", gaps)
    assert len(vA) >= 2 and len(gaps) == min(3, len(vA)) and min(gaps) > 1e-6
    vB, ccB = _st_run(g, tmp_path, St=St_ref)
    assert vA == vB
    assert ccA.numComp == ccB.numComp and ccA.comps.shape == ccB.comps.shape
    scale0 = np.linalg.norm(np.multiply.outer(ccB.weigs[:, 0], ccB.comps[0]))
    for k in range(ccB.comps.shape[0]):
        a = np.multiply.outer(ccA.weigs[:, k], ccA.comps[k])
        b = np.multiply.outer(ccB.weigs[:, k], ccB.comps[k])
        if np.linalg.norm(b) < 1e-9 * scale0:
            continue
        assert np.linalg.norm(a - b) / np.linalg.norm(b) < 1e-6, k
    n = min(8, ccB.weigs.shape[1])
    assert np.linalg.norm(ccA.weigs[:, :n] - ccB.weigs[:, :n]) / np.linalg.norm(ccB.weigs[:, :n]) < 1e-9


def test_without_wi_nothing_is_left():
    g = _g("tets_strain")[0]
    from animsnapbases_amd import nonlinearSnapshots
    snaps = _snaps(g["frames"][:5])
    ns = nonlinearSnapshots.from_positions(_st_param("."), snaps, "tets_strain", g["elements"], rest_positions=g["rest"])
    assert ns.assembly_ST is None and snaps.assembly_ST is None


# ------------------------------------------------------------------ 8. adoption by the position path
def test_force_snapshots_go_into_the_position_path():
    from animsnapbases_amd import posSnapshots
    g = _g("tets_strain")[0]
    out, F = _snaps(g["frames"]).constraint_forces([_spec("tets_strain")])
    N = out.shape[1]
    b = out.cpu().numpy()                                           # (from_device standardises the tensor in place)
    with contextlib.redirect_stdout(io.StringIO()):
        fs = posSnapshots.from_device(out.data_ptr(), F, N, rest_shape="first", standarize=True, keepalive=out)
    assert (fs.frs, fs.nVerts) == (F, N)
    T = fs.snapTensor
    assert T.shape == (F, N, 3)
    back = T / fs.pre_scale_factor + fs.mean
    scale = np.abs(b).max()
    err = np.abs(back - b).max()
    print("adoption: max abs err %.3g of %.3g" % (err, scale))
    # |b - mean| <= 2 scale; subtracting the mean row, the scaling (by a rounded reciprocal) and its inverse round once each
    # at that size, the final sum once at |b|: 9 eps scale, 16 with a margin
    assert err <= 16 * EPS * scale


# ------------------------------------------------------------------ 9. refusals
def test_refusals():
    g = _g("tets_strain")[0]
    snaps = _snaps(g["frames"][:3])
    tets = _spec("tets_strain")
    with pytest.raises(ValueError, match="non-empty list"):
        snaps.constraint_forces([])
    with pytest.raises(ValueError, match="unknown projection kind"):
        snaps.constraint_forces([dict(tets, kind="tets_stress")])
    with pytest.raises(ValueError, match="sigma_min"):
        snaps.constraint_forces([dict(tets, sigma_min=1.1, sigma_max=0.9)])
    for rng in (dict(frame_start=2, frame_end=2), dict(frame_start=3), dict(frame_end=4), dict(frame_jump=0)):
        with pytest.raises(ValueError, match="empty frame range"):
            snaps.constraint_forces([tets], **rng)
    with pytest.raises(ValueError, match=r"\(n, 2\) expected"):
        snaps.constraint_forces([tets, dict(kind="edge_spring", elements=g["elements"])])
    with pytest.raises(ValueError, match="finite"):
        snaps.constraint_forces([dict(tets, wi=float("inf"))])
    assert snaps.assembly_ST is None


def test_a_thread_rank_group_of_two_is_refused():
    from animsnapbases_amd import HipEngine
    from thread_comm import run_ranks
    g = _g("tets_strain")[0]

    def run(rank, comm):
        from animsnapbases_amd import posSnapshots
        with contextlib.redirect_stdout(io.StringIO()):
            snaps = posSnapshots.from_arrays(np.array(g["frames"][:3]), None, "first", standarize=False, massWeight=False,
                                             engine=HipEngine(0, stream=0), comm=comm)
        with pytest.raises(NotImplementedError, match="several ranks"):
            snaps.constraint_forces([_spec("tets_strain")])
        return True

    assert run_ranks(2, run) == [True, True]


def test_the_c_entry_checks_the_csr():
    """asb_cforce_run refuses a CSR that does not fit the set-up before any kernel runs."""
    import torch
    from animsnapbases_amd import projections as proj
    g = _g("tets_strain")[0]
    N = g["rest"].shape[0]
    snaps = _snaps(g["frames"][:3])
    eng = snaps._engine
    setup = proj.build_setup("tets_strain", g["elements"][:5], g["rest"])
    St = proj.assembly_ST(setup, N, 0.7)
    eng.cproj_setup(setup)
    out = torch.zeros((3, N, 3), dtype=torch.float64, device="cuda:%d" % eng.device_id)
    args = (0, 0, 3, 1, None, False, 1.0, 1.0, 1.0)
    wide = proj.assembly_ST(proj.build_setup("tets_strain", g["elements"][:6], g["rest"]), N, 0.7)
    v = int(np.argmax(np.diff(St.indptr)))                          # a row with several entries, its first two swapped
    idx = St.indices.copy()
    idx[St.indptr[v]:St.indptr[v] + 2] = idx[St.indptr[v]:St.indptr[v] + 2][::-1]
    unsorted = sparse.csr_matrix((St.data, idx, St.indptr), shape=St.shape)
    for bad, what in ((wide, "names column"), (St[:N - 1], "rows"), (unsorted, "ascending")):
        with pytest.raises(RuntimeError, match=what):
            eng.cforce_run(*args, bad, False, 0, out.data_ptr())
    assert (out == 0).all().item()
    eng.cforce_run(*args, St, False, 0, out.data_ptr())
    assert (out != 0).any().item()
