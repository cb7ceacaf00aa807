"""GPU (-m gpu): the constraint-basis variants that need S^T or block interpolation, on several ranks.  Each rank of
``thread_comm.run_ranks`` owns its own HipEngine on device 0 and the collectives are emulated; the torch.distributed wiring
runs as two gloo processes under the launcher (tests/st_multirank_driver.py).  Everything a run returns must equal the
one-rank run bit for bit (the |R| column of the measures, a sum over ranks, to 1e-12), on every rank."""
import contextlib
import io
import os
import socket
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import load_golden, relerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _param(tmp, p, basis, kind="geom", K=0, ele="_tris", snaps="tris_strain", store=True, standarize=True):
    return types.SimpleNamespace(constProj_rest_shape="first", constProj_numFrames=0, constProj_p_size=p,
                                 constProj_massWeight=False, constProj_standarize=standarize, constProj_orthogonal=False,
                                 constProj_basis_type=basis, deim_desired_num_components=K, constProj_store_sing_val=store,
                                 constProj_support="global", constProj_output_directory=str(tmp), name="st", constProj_name="mr",
                                 constProj_bases_interpolation_type=kind, constProj_snapshots_type=snaps,
                                 constProj_element_type=ele, bases_R_tol=1e-8, geom_ele_per_vert=2)


def _setup(param, frames, St=None, elems=None, engine=None, comm=None, comps=None, K=0):
    from animsnapbases_amd import constraintsComponents, nonlinearSnapshots
    ns = nonlinearSnapshots(param, frames=frames, engine=engine, comm=comm)
    ns.config()
    if elems is not None:
        if param.constProj_element_type == "_edges":
            ns.edges = elems
        else:
            ns.tris = elems
    ns.snapshots_prepare()
    cc = constraintsComponents(param, ns)
    cc.config()
    cc.St = St
    if comps is not None:
        cc.numComp, cc.comps = K, comps
    return ns, cc


def _ranks(world, fn):
    from animsnapbases_amd import HipEngine
    from thread_comm import run_ranks
    with contextlib.redirect_stdout(io.StringIO()):
        return run_ranks(world, lambda rank, comm: fn(HipEngine(0, stream=0), comm))


def _golden_st(g):
    from scipy import sparse
    return sparse.csr_matrix((g["St_data"], g["St_indices"], g["St_indptr"]), shape=tuple(g["St_shape"]))


def _st_outputs(cc):
    return dict(verts=cc.largeDeforPoints.copy(), blocks=cc.largeDeforBlocks.copy(), comps=cc.comps.copy(), weigs=cc.weigs.copy(),
                meas=cc.measures_at_largeDeforVerts.copy(), numComp=cc.numComp, halo=cc.st_halo_rows)


def _same_st(a, b):
    for k in ("verts", "blocks", "comps", "weigs"):
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.int64), b[k].view(np.int64)), k
    assert a["numComp"] == b["numComp"]
    m, n = a["meas"], b["meas"]
    assert m.shape == n.shape
    assert np.array_equal(m[:, :2], n[:, :2]) and np.array_equal(m[:, 3:], n[:, 3:])
    assert np.all(np.abs(m[:, 2] - n[:, 2]) <= 1e-12 * np.abs(n[:, 2]))


def _run_st(cc):
    with contextlib.redirect_stdout(io.StringIO()):
        cc.compute_components_store_singvalues()
    return _st_outputs(cc)


@pytest.mark.parametrize("world", [2, 3])
def test_pca_blocks_with_St_golden_several_ranks(world, tmp_path):
    g = load_golden("with_st_p2")
    p = int(g["p"])
    St = _golden_st(g)
    os.makedirs(str(tmp_path / "one"))
    one = _run_st(_setup(_param(tmp_path / "one", p, "pca_blocks_with_St"), g["frames"], St, g["tris"])[1])

    def rank(eng, comm):
        _, cc = _setup(_param(tmp_path, p, "pca_blocks_with_St"), g["frames"], St, g["tris"], engine=eng, comm=comm)
        return _run_st(cc)
    outs = _ranks(world, rank)
    for out in outs:
        _same_st(out, one)
        assert len(out["halo"]) == world and out["halo"] == outs[0]["halo"]
        assert out["verts"].tolist() == g["st_verts"].tolist()
        comps, weigs = out["comps"], out["weigs"].copy()
        for k in range(comps.shape[0]):
            if np.vdot(weigs[:, k], g["st_weigs"][:, k]) < 0:
                weigs[:, k] *= -1
        scale0 = np.linalg.norm(np.multiply.outer(g["st_weigs"][:, 0], g["st_comps"][0]))
        for k in range(comps.shape[0]):
            b = np.multiply.outer(g["st_weigs"][:, k], g["st_comps"][k])
            if np.linalg.norm(b) >= 1e-9 * scale0:
                assert relerr(np.multiply.outer(out["weigs"][:, k], comps[k]), b) < 1e-6, k
        assert relerr(weigs[:, :8], g["st_weigs"][:, :8]) < 1e-9
        m, mr = out["meas"], g["st_measures"]
        assert np.array_equal(m[:, :2], mr[:, :2])
        big = mr[:, 2] > 1e-6 * mr[0, 2]
        assert relerr(m[big, 2:], mr[big, 2:]) < 1e-8
    rows = open(str(tmp_path / "st_mr_constrprojBases_pcaExtraction_singValues.csv")).read().splitlines()
    assert len(rows) == 1 + outs[0]["meas"].shape[0]          # rank 0 wrote it


def _geom_outputs(cc):
    return [np.asarray(x).tolist() for x in (cc.geom_interpol_verts, cc.geom_alpha, cc.geom_Pt, cc.geom_alpha_ranges)]


@pytest.mark.parametrize("world", [2, 4])
def test_position_space_geom_golden_several_ranks(world, tmp_path):
    g = load_golden("with_st_p2")
    p, K = int(g["p"]), int(g["pos_K"])
    St = _golden_st(g)
    _, cc = _setup(_param(tmp_path, p, "pca_blocks", K=K, store=False), g["frames"], St, g["tris"])
    with contextlib.redirect_stdout(io.StringIO()):
        cc.compute_components_store_singvalues()
        V = cc.comps.copy()
        cc.geom_block_form_utilizing_differential_operator(True)
    one = _geom_outputs(cc)
    assert one == [g[k].tolist() for k in ("pos_interpol_verts", "pos_alpha", "pos_Pt", "pos_ranges")]

    def rank(eng, comm):
        _, c = _setup(_param(tmp_path, p, "pca_blocks", K=K, store=False), g["frames"], St, g["tris"], engine=eng, comm=comm,
                      comps=V, K=K)
        c.geom_block_form_utilizing_differential_operator(True)
        return _geom_outputs(c), c.st_halo_rows
    outs = _ranks(world, rank)
    for out, halo in outs:
        assert out == one
        assert len(halo) == world and sum(halo) > 0


@pytest.mark.parametrize("world", [2, 4])
def test_block_interpolation_golden_several_ranks(world, tmp_path):
    g = load_golden("block_deim_p3")
    K, p = int(g["K"]), int(g["p"])

    def rank(eng, comm):
        res = {}
        for kind in ("deim_block_form", "geom"):
            _, cc = _setup(_param(tmp_path, p, "pca_blocks", kind, K, store=False), g["frames"], engine=eng, comm=comm)
            cc.compute_components_store_singvalues()
            if kind == "deim_block_form":
                cc.deim_blocksForm()
            else:
                cc.geom_block_form_utilizing_differential_operator(False)
            res[kind] = [cc.geom_Pt.tolist(), cc.geom_alpha.tolist(), cc.geom_alpha_ranges.tolist()]
        return res
    for out in _ranks(world, rank):
        for kind in ("deim_block_form", "geom"):
            assert out[kind] == [g[kind + "_Pt"].tolist(), g[kind + "_alpha"].tolist(), g[kind + "_ranges"].tolist()], kind


def test_block_interpolation_shard_rule(tmp_path):
    """120 rows over 3 ranks are not whole constraints of 3 rows: the constraint-space geom refuses, row-wise block DEIM
    (arg-max over rows) still runs and matches the golden."""
    g = load_golden("block_deim_p3")
    K, p = int(g["K"]), int(g["p"])
    _, cc = _setup(_param(tmp_path, p, "pca_blocks", "deim_block_form", K, store=False), g["frames"])
    with contextlib.redirect_stdout(io.StringIO()):
        cc.compute_components_store_singvalues()
    V = cc.comps.copy()

    def rank(eng, comm):
        _, c = _setup(_param(tmp_path, p, "pca_blocks", "deim_block_form", K, store=False), g["frames"], engine=eng, comm=comm,
                      comps=V, K=K)
        c.deim_blocksForm()
        got = [c.geom_Pt.tolist(), c.geom_alpha.tolist(), c.geom_alpha_ranges.tolist()]
        with pytest.raises(ValueError, match="shards of whole constraints"):
            c.geom_block_form_utilizing_differential_operator(False)
        return got
    for got in _ranks(3, rank):
        assert got == [g["deim_block_form_Pt"].tolist(), g["deim_block_form_alpha"].tolist(), g["deim_block_form_ranges"].tolist()]


@pytest.mark.parametrize("world", [2, 3])
def test_geom_constructed_several_ranks(world, tmp_path):
    g = load_golden("pod_deim_small")
    rec = load_golden("pod_deim_recon")
    K = int(g["K"])
    param = _param(tmp_path, 1, "pod_vectorized", "deim", K, store=False)
    ns, cc = _setup(param, g["frames"])
    with contextlib.redirect_stdout(io.StringIO()):
        cc.compute_components_store_singvalues()
        cc.deim()
    ns.test_snapTensor = rec["test_snapTensor"]
    assert cc.geom_Pt.tolist() == rec["Pt"].tolist()
    V, alpha, ranges = cc.comps.copy(), cc.geom_alpha.copy(), cc.geom_alpha_ranges.copy()
    cases = [(r, case) for r in (3, K) for case in ("train", "test")]
    one = [cc.geom_constructed(r, case) for r, case in cases]
    for (r, case), x in zip(cases, one):
        assert relerr(x, rec["%s_r%d" % (case, r)]) < 1e-8

    def rank(eng, comm):
        ns_, c = _setup(_param(tmp_path, 1, "pod_vectorized", "deim", K, store=False), g["frames"], engine=eng, comm=comm,
                        comps=V, K=K)
        ns_.test_snapTensor = rec["test_snapTensor"]
        c.geom_alpha, c.geom_Pt, c.geom_alpha_ranges = alpha, alpha, ranges
        return [c.geom_constructed(r, case) for r, case in cases]
    for out in _ranks(world, rank):
        for a, b in zip(out, one):
            assert a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---------------------------------------------------------------------------------------- a larger synthetic mesh
def _grid(n):
    """n x n vertices, 2 (n-1)^2 triangles, their edges."""
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a = (i * n + j).ravel()
    tris = np.stack([np.stack([a, a + n, a + 1], 1), np.stack([a + 1, a + n, a + n + 1], 1)], 1).reshape(-1, 3)     # cell by cell
    e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [0, 2]]])
    edges = np.unique(np.sort(e, axis=1), axis=0)
    return tris.astype(np.int64), edges.astype(np.int64)


def _synthetic(kind, permuted, F, rank_, seed):
    from scipy import sparse
    rng = np.random.default_rng(seed)
    n = 200
    tris, edges = _grid(n)
    elems = tris if kind == "_tris" else edges
    if permuted:
        elems = elems[rng.permutation(elems.shape[0])]
    p = 2 if kind == "_tris" else 1
    e = elems.shape[0]
    rows = np.repeat(elems.ravel(), p).reshape(-1)                     # vertex of every (element, corner, constraint row)
    cols = (np.repeat(np.arange(e), elems.shape[1])[:, None] * p + np.arange(p)[None, :]).reshape(-1)
    St = sparse.csr_matrix((rng.uniform(0.5, 1.5, size=rows.shape[0]), (rows, cols)), shape=(n * n, e * p))
    modes = rng.normal(size=(rank_, e * p * 3))
    frames = (rng.normal(size=(F, rank_)) @ modes).reshape(F, e * p, 3)
    return frames, St, elems, p


@pytest.mark.parametrize("kind,F,rank_", [("_tris", 64, 20), ("_edges", 128, 14)])
@pytest.mark.parametrize("permuted", [False, True])
def test_synthetic_mesh_equals_one_rank(kind, F, rank_, permuted, tmp_path):
    import torch
    from animsnapbases_amd.distributed import partition
    frames, St, elems, p = _synthetic(kind, permuted, F, rank_, 7 + F)
    snaps = "tris_strain" if kind == "_tris" else "edge_spring"

    # (not standardised: the mean and variance are sums all-reduced over the ranks, which can round differently in the last
    # bit for another world size -- the prepared tensor itself would then differ, before any S^T work)
    def prm():
        return _param(tmp_path, p, "pca_blocks_with_St", ele=kind, snaps=snaps, store=False, standarize=False)
    ns, cc = _setup(prm(), frames, St, elems)
    one = _run_st(cc)
    assert np.isfinite(one["comps"]).all() and one["verts"].shape[0] >= 1
    K = one["numComp"]
    with contextlib.redirect_stdout(io.StringIO()):
        cc.geom_block_form_utilizing_differential_operator(True)
    one_geom = _geom_outputs(cc)
    del ns, cc

    def rank(eng, comm):
        _, c = _setup(prm(), frames, St, elems, engine=eng, comm=comm)
        c.compute_components_store_singvalues()
        out = _st_outputs(c)
        plan = c._st_plan
        out["halo_ids"], out["send"] = plan["halo"], plan["send"]
        out["H"] = eng.st_halo_download(0)
        L = eng.xchg_len() - 2
        buf = torch.zeros(max(1, len(plan["send"])) * L, dtype=torch.float64, device="cuda")
        eng.st_halo_pack(0, plan["send"], buf.data_ptr())
        out["own"] = buf.cpu().numpy()[:len(plan["send"]) * L].reshape(len(plan["send"]), 3, L // 3)[:, :, :F]
        c.geom_block_form_utilizing_differential_operator(True)
        out["geom"] = _geom_outputs(c)
        return out
    for world in (2, 4):
        outs = _ranks(world, rank)
        shards = partition(frames.shape[1], world)
        for r, out in enumerate(outs):
            _same_st(out, one)
            assert out["geom"] == one_geom
            assert out["halo"] == [len(o["halo_ids"]) for o in outs]
            # every halo row equals its owner's residual row bit for bit
            for i, gidx in enumerate(out["halo_ids"]):
                q = max(k for k, (a, _) in enumerate(shards) if a <= gidx)
                j = int(np.searchsorted(outs[q]["send"], gidx))
                assert np.array_equal(out["H"][i].view(np.int64), outs[q]["own"][j].view(np.int64)), (r, gidx)
        h = sum(outs[0]["halo"])
        if permuted:
            assert h > 0.3 * frames.shape[1]
        else:
            assert 0 < h < 0.05 * frames.shape[1]
    assert K >= 1


# ---------------------------------------------------------------------------------------- torch.distributed, two processes
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_processes_gloo(tmp_path):
    g = load_golden("with_st_p2")
    p, K = int(g["p"]), int(g["pos_K"])
    St = _golden_st(g)
    one = _run_st(_setup(_param(tmp_path, p, "pca_blocks_with_St"), g["frames"], St, g["tris"])[1])
    _, cc = _setup(_param(tmp_path, p, "pca_blocks", K=K, store=False), g["frames"], St, g["tris"])
    with contextlib.redirect_stdout(io.StringIO()):
        cc.compute_components_store_singvalues()
        cc.geom_block_form_utilizing_differential_operator(True)
    one_geom = _geom_outputs(cc)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    out = tmp_path / "out"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "st_multirank_driver.py"), str(out)]
    pr = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert pr.returncode == 0, pr.stderr.decode(errors="replace")[-4000:]
    for r in range(2):
        d = np.load(str(out / ("rank%d.npz" % r)))
        for k in ("verts", "blocks", "comps", "weigs"):
            assert np.array_equal(d[k].view(np.int64), one[k].view(np.int64)), (r, k)
        assert np.array_equal(d["meas"][:, :2], one["meas"][:, :2]) and np.array_equal(d["meas"][:, 3:], one["meas"][:, 3:])
        assert np.all(np.abs(d["meas"][:, 2] - one["meas"][:, 2]) <= 1e-12 * np.abs(one["meas"][:, 2]))
        assert [d[k].tolist() for k in ("g_verts", "g_alpha", "g_Pt", "g_ranges")] == one_geom
