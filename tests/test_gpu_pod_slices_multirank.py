"""GPU (-m gpu): constProj_basis_type 'pod' (the per-(p, d) slice POD, constraintsComponents.py:274-294) with the constraint
rows sharded over several ranks: partial Gram matrices all-reduced, slice s solved by rank s % W, every slice's V S^-1 handed
over through one all-reduced buffer, each rank forming its own basis rows.  The ranks of ``thread_comm.run_ranks`` share
device 0 with emulated collectives; the torch.distributed wiring runs as two gloo processes under the launcher
(tests/pod_slices_multirank_driver.py)."""
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


def _param(tmp, p, K, orthogonal=False):
    return types.SimpleNamespace(constProj_rest_shape="first", constProj_numFrames=0, constProj_p_size=p,
                                 constProj_massWeight=False, constProj_standarize=True, constProj_orthogonal=orthogonal,
                                 constProj_basis_type="pod", deim_desired_num_components=K, constProj_store_sing_val=False,
                                 constProj_output_directory=str(tmp), name="t", constProj_name="pod",
                                 constProj_bases_interpolation_type="deim", constProj_snapshots_type="tris_strain")


def _setup(param, frames, engine=None, comm=None, phased=False):
    from animsnapbases_amd import constraintsComponents, nonlinearSnapshots
    with contextlib.redirect_stdout(io.StringIO()):
        ns = nonlinearSnapshots(param, frames=frames, engine=engine, comm=comm)
        ns.config()
        ns.snapshots_prepare()
        cc = constraintsComponents(param, ns)
        cc.config()
    cc._phased_pod_slices = phased
    return ns, cc


def _pod(param, frames, engine=None, comm=None, phased=False):
    ns, cc = _setup(param, frames, engine, comm, phased)
    with contextlib.redirect_stdout(io.StringIO()):
        cc.compute_components_store_singvalues()
    return ns, cc


def _ranks(world, fn):
    from animsnapbases_amd import HipEngine
    from thread_comm import run_ranks
    with contextlib.redirect_stdout(io.StringIO()):
        return run_ranks(world, lambda rank, comm: fn(HipEngine(0, stream=0), comm))


def _slice_vectors(comps, p):
    """(pi, d, k) -> the k-th vector of slice (pi, d): comps[k, pi::p, d]."""
    K = comps.shape[0]
    return {(pi, d, k): comps[k, pi::p, d] for pi in range(p) for d in range(3) for k in range(K)}


def _same_up_to_sign(a, b, p, tol):
    va, vb = _slice_vectors(a, p), _slice_vectors(b, p)
    for key in va:
        x, y = va[key], vb[key]
        assert relerr(x * np.sign(np.dot(x, y)), y) <= tol, key


def _check_against_svd(comps, X, p, K, tol, ref32=None):
    """Every slice vector against NumPy's float64 SVD of the slice (and the reference's float32 result)."""
    for pi in range(p):
        for d in range(3):
            U = np.linalg.svd(X[:, pi::p, d].T, full_matrices=False)[0][:, :K].T
            for k in range(K):
                got = comps[k, pi::p, d]
                assert relerr(got * np.sign(np.dot(got, U[k])), U[k]) < tol, (pi, d, k)
                if ref32 is not None:
                    r = ref32[k, pi::p, d]
                    assert relerr(got * np.sign(np.dot(got, r)), r) < 2e-4, (pi, d, k)


def _low_rank(seed, F, rows, rank_, decay, noise):
    rng = np.random.default_rng(seed)
    modes = rng.normal(size=(rank_, rows, 3))
    coef = rng.normal(size=(F, rank_)) * (decay ** np.arange(rank_))[None]
    return 0.2 + np.tensordot(coef, modes, (1, 0)) + noise * rng.normal(size=(F, rows, 3))


@pytest.mark.parametrize("world", [2, 3, 4])
def test_golden_several_ranks(world, tmp_path):
    """72 rows, p = 2: shards of 36 / 24 / 18 rows hold whole constraints."""
    g = load_golden("pod_slices_p2")
    K, p = int(g["K"]), int(g["p"])
    ns1, cc1 = _pod(_param(tmp_path, p, K), g["frames"])
    one, X = cc1.comps.copy(), ns1.snapTensor.copy()

    def rank(eng, comm):
        _, cc = _pod(_param(tmp_path, p, K), g["frames"], engine=eng, comm=comm)
        return cc.comps.copy(), cc.numComp
    outs = _ranks(world, rank)
    for comps, nc in outs:
        assert nc == K and comps.shape == g["comps"].shape
        assert np.array_equal(comps.view(np.int64), outs[0][0].view(np.int64))        # every rank: the same bits
    comps = outs[0][0]
    _check_against_svd(comps, X, p, K, 1e-8, g["comps"])
    _same_up_to_sign(comps, one, p, 1e-10)


def test_more_ranks_than_slices(tmp_path):
    """p = 1: three slices over four ranks -- rank 3 owns none and only takes part in the collectives."""
    K, p = 6, 1
    frames = _low_rank(11, 24, 80, 9, 0.7, 1e-3)
    ns1, _ = _pod(_param(tmp_path, p, K), frames)
    X = ns1.snapTensor.copy()

    def rank(eng, comm):
        _, cc = _pod(_param(tmp_path, p, K), frames, engine=eng, comm=comm)
        return cc.comps.copy()
    outs = _ranks(4, rank)
    for comps in outs:
        assert comps.shape == (K, 80, 3)
        assert np.array_equal(comps.view(np.int64), outs[0].view(np.int64))
    _check_against_svd(outs[0], X, p, K, 1e-8)


def test_shard_rule(tmp_path):
    """72 rows, p = 2 over five ranks (15 / 15 / 14 / 14 / 14 rows): no shard of whole constraints -- every rank refuses."""
    g = load_golden("pod_slices_p2")
    K, p = int(g["K"]), int(g["p"])

    def rank(eng, comm):
        _, cc = _setup(_param(tmp_path, p, K), g["frames"], engine=eng, comm=comm)
        with pytest.raises(ValueError, match="shards of whole constraints"):
            cc.compute_components_store_singvalues()
        return True
    assert _ranks(5, rank) == [True] * 5


def test_refusal_agrees(tmp_path):
    """Slice 5 (p_i = 1, d = 2) of rank 2 < K: one rank and two / three ranks raise the same error naming it."""
    g = load_golden("pod_slices_p2")
    K, p = int(g["K"]), int(g["p"])
    frames = g["frames"].copy()
    rng = np.random.default_rng(3)
    frames[:, 1::p, 2] = 0.5 + rng.normal(size=(frames.shape[0], 2)) @ rng.normal(size=(2, frames.shape[1] // p))
    _, cc = _setup(_param(tmp_path, p, K), frames)
    with pytest.raises(RuntimeError) as one:
        with contextlib.redirect_stdout(io.StringIO()):
            cc.compute_components_store_singvalues()
    msg = str(one.value)
    assert "pod: slice 5 has fewer than %d singular values" % K in msg

    def rank(eng, comm):
        _, c = _setup(_param(tmp_path, p, K), frames, engine=eng, comm=comm)
        with pytest.raises(RuntimeError) as exc:
            c.compute_components_store_singvalues()
        return str(exc.value)
    for world in (2, 3):
        assert _ranks(world, rank) == [msg] * world


@pytest.mark.parametrize("case", ["golden", "p3"])
def test_phased_path_on_one_rank_is_bit_identical(case, tmp_path):
    """The phases (Gram matrices -> eigen-solve into the exchange slot -> basis) make the same GEMM and eigen-solver calls on
    the same data as asb_pod_slices: the same basis bit for bit."""
    if case == "golden":
        g = load_golden("pod_slices_p2")
        frames, K, p = g["frames"], int(g["K"]), int(g["p"])
    else:
        frames, K, p = _low_rank(5, 40, 150, 16, 0.8, 1e-4), 12, 3
    _, cc = _pod(_param(tmp_path, p, K), frames)
    ref = cc.comps.copy()
    _, cp = _pod(_param(tmp_path, p, K), frames, phased=True)
    assert cp.numComp == K
    assert np.array_equal(cp.comps.view(np.int64), ref.view(np.int64))


@pytest.mark.parametrize("orthogonal", [False, True])
def test_downstream_deim_on_two_ranks(orthogonal, tmp_path):
    """pod -> post_process_components -> deim() on two ranks picks the points one rank picks for that basis.  (Each slice
    vector carries an arbitrary sign, as in the reference's SVD; the device eigen-solver's sign can differ between the
    one-rank and the all-reduced Gram matrix, and a flipped slice vector changes the component -- so one rank runs the
    post-processing and the device DEIM loop on the basis the two ranks computed.)"""
    g = load_golden("pod_slices_p2")
    K, p = int(g["K"]), int(g["p"])
    _, cc = _pod(_param(tmp_path, p, K, orthogonal), g["frames"])
    one = cc.comps.copy()

    def rank(eng, comm):
        _, c = _pod(_param(tmp_path, p, K, orthogonal), g["frames"], engine=eng, comm=comm)
        raw = c.comps.copy()
        c.post_process_components()
        c.deim()
        return raw, [c.geom_Pt.tolist(), c.geom_alpha.tolist(), c.geom_alpha_ranges.tolist()]
    outs = _ranks(2, rank)
    raw = outs[0][0]
    assert np.array_equal(raw.view(np.int64), outs[1][0].view(np.int64))
    _same_up_to_sign(raw, one, p, 1e-10)
    _, c1 = _setup(_param(tmp_path, p, K, orthogonal), g["frames"])
    c1.comps, c1.numComp = raw, K
    with contextlib.redirect_stdout(io.StringIO()):
        c1.post_process_components()
        c1.deim()
    ref = [c1.geom_Pt.tolist(), c1.geom_alpha.tolist(), c1.geom_alpha_ranges.tolist()]
    assert len(ref[0]) == K and len(set(ref[0])) == K
    assert [pts for _, pts in outs] == [ref, ref]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_processes_gloo(tmp_path):
    """Two processes, a gloo group (F = 14: far below the co-resident tridiagonalisation kernel's size)."""
    g = load_golden("pod_slices_p2")
    K, p = int(g["K"]), int(g["p"])
    _, cc = _pod(_param(tmp_path, p, K), g["frames"])
    one = cc.comps.copy()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    out = tmp_path / "out"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "pod_slices_multirank_driver.py"), str(out)]
    pr = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert pr.returncode == 0, pr.stderr.decode(errors="replace")[-4000:]
    got = [np.load(str(out / ("rank%d.npz" % r)))["comps"] for r in range(2)]
    assert np.array_equal(got[0].view(np.int64), got[1].view(np.int64))
    for comps in got:
        assert comps.shape == one.shape
        _same_up_to_sign(comps, one, p, 1e-10)
