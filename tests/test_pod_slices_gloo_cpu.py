"""CPU, gloo world 2 / 3: the host protocol of constProj_basis_type 'pod' on several ranks
(constraintsComponents._pod_slices_phased) driven through a NumPy stand-in of the engine's three phase methods.  Checks:
slice ownership (slice s solved by rank s % W only), the hand-over through the all-reduced buffer (every rank holds the
owner's bits), the basis against NumPy's SVD of every slice, and that every rank refuses a rank-deficient slice alike."""
import ctypes
import os
import socket
import sys
import types

import numpy as np
import pytest

from conftest import ROOT


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _view(ptr, n):
    return np.ctypeslib.as_array((ctypes.c_double * int(n)).from_address(int(ptr)))


class _NumpyPodEngine(object):
    """The phase methods of HipEngine on host arrays: X (3 n_loc, F), rows 3 v + d of this shard's constraints."""
    device_exchange = False

    def __init__(self, X_loc):
        self.X = np.ascontiguousarray(X_loc.transpose(1, 2, 0).reshape(-1, X_loc.shape[0]))
        self.F, self.n_loc, self.K = X_loc.shape[0], X_loc.shape[1], 0
        self.solved, self.vs = [], None

    def pod_slice_grams(self, p, s0, ns, G_ptr):
        G = _view(G_ptr, ns * self.F * self.F).reshape(ns, self.F, self.F)
        for i in range(ns):
            M = self.X[s0 + i::3 * p]
            G[i] = M.T @ M

    def pod_slice_eig(self, K, G_ptr, VS_ptr, st_ptr):
        G = _view(G_ptr, self.F * self.F).reshape(self.F, self.F)
        lam, V = np.linalg.eigh(G)
        lam, V = lam[::-1][:K], V[:, ::-1][:, :K]
        ok = lam > 1e-14 * lam[0]
        _view(VS_ptr, self.F * K)[:] = np.where(ok[None, :], V / np.sqrt(np.where(ok, lam, 1.0))[None, :], 0.0).reshape(-1)
        _view(st_ptr, 1)[0] = 0.0 if ok.all() else 1.0
        self.solved.append(G_ptr)

    def pod_slices_basis(self, p, K, VS_ptr):
        S = 3 * p
        buf = _view(VS_ptr, S * self.F * K + S)
        self.vs = buf.copy()
        bad = np.flatnonzero(buf[S * self.F * K:])
        if bad.size:
            raise RuntimeError("pod: slice %d has fewer than %d singular values above 1e-7 of its largest" % (bad[0], K))
        comps = np.empty((K, 3 * self.n_loc))
        for s in range(S):
            comps[:, s::S] = (self.X[s::S] @ buf[s * self.F * K:(s + 1) * self.F * K].reshape(self.F, K)).T
        self.comps = comps.reshape(K, self.n_loc, 3)
        self.K = K

    def sync(self):
        pass

    def results_comps(self):
        return self.comps


def _frames(deficient):
    rng = np.random.default_rng(17)
    F, rows = 20, 72
    frames = rng.normal(size=(F, 9)) @ rng.normal(size=(9, rows * 3)) + 1e-3 * rng.normal(size=(F, rows * 3))
    frames = frames.reshape(F, rows, 3)
    if deficient:
        frames[:, 1::2, 2] = rng.normal(size=(F, 2)) @ rng.normal(size=(2, rows // 2))     # slice 5 of p = 2: rank 2
    return frames


def _worker(rank, world, port, tmpdir):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.chdir(tmpdir)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        from animsnapbases_amd import Comm, constraintsComponents, nonlinearSnapshots
        comm = Comm()
        p, K = 2, 5
        out = {}
        for deficient in (False, True):
            frames = _frames(deficient)
            F, N = frames.shape[0], frames.shape[1]
            v0, n = comm.my_shard(N)
            param = types.SimpleNamespace(deim_desired_num_components=K, constProj_output_directory=tmpdir)
            eng = _NumpyPodEngine(frames[:, v0:v0 + n])
            ns = nonlinearSnapshots(param, engine=eng, comm=comm)
            ns.constraintsSize, ns.frs, ns.frames_rows, ns._shards = p, F, N, comm.shards(N)
            cc = constraintsComponents(param, ns)
            if deficient:
                with pytest.raises(RuntimeError) as exc:
                    cc.compute_pod_for_nonlinear_snapshots_tensor()
                out["refusal"] = np.array(str(exc.value))
            else:
                cc.compute_pod_for_nonlinear_snapshots_tensor()
                out["comps"], out["vs"] = cc.comps, eng.vs
                out["n_solved"] = np.array(len(eng.solved))
        np.savez(os.path.join(tmpdir, "rank%d.npz" % rank), **out)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_pod_slices_protocol_gloo(world, tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    res = [np.load(str(tmp_path / ("rank%d.npz" % r))) for r in range(world)]
    p, K, S = 2, 5, 6
    # ownership: rank r solved the slices s with s % world == r
    assert [int(d["n_solved"]) for d in res] == [len(range(r, S, world)) for r in range(world)]
    # hand-over: one buffer, the owner's bits on every rank
    for d in res[1:]:
        assert np.array_equal(d["vs"].view(np.int64), res[0]["vs"].view(np.int64))
        assert np.array_equal(d["comps"].view(np.int64), res[0]["comps"].view(np.int64))
    X = _frames(False)
    comps = res[0]["comps"]
    for pi in range(p):
        for d in range(3):
            U = np.linalg.svd(X[:, pi::p, d].T, full_matrices=False)[0][:, :K].T
            for k in range(K):
                got = comps[k, pi::p, d]
                assert np.linalg.norm(got * np.sign(got @ U[k]) - U[k]) < 1e-9, (pi, d, k)
    assert all(str(d["refusal"]) == "pod: slice 5 has fewer than 5 singular values above 1e-7 of its largest" for d in res)
