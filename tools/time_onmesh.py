"""Timing of the on-mesh accuracy maps (posComponents.on_mesh_accuracy, csrc/asb_onmesh.hip) at config 4's shape: a triangulated
grid of 100 000 vertices (250 x 400) x 2 000 frames, displaced by smooth modes plus noise, r = K = 64, all frames.

Legs, each in a child process of its own under a time limit; the first failure ends the run:
  errors   normals=False: the error pass (one read of the tensor)
  normals  normals=True: error pass + normal pass
  host     for scale only, on a SUBSAMPLE of at most 5 000 vertices (a 50 x 100 corner of the grid with its own triangles): the
           route without this path -- download snapTensor, tensordot, the measures per frame in NumPy on the host's cores
Device legs: best of 3 after a warm-up, device events on the engine's stream (the null stream) around the C call, which ends in
the download of the (N,) and (F,) results.

  python tools/time_onmesh.py [--n0 250] [--n1 400] [--frames 2000] [--k 64] [--leg errors|normals|host]
"""
import argparse
import contextlib
import io
import json
import os
import subprocess
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def grid(n0, n1, h=0.05):
    x, y = np.meshgrid(np.arange(n0) * h, np.arange(n1) * h, indexing="ij")
    rest = np.stack([x.ravel(), y.ravel(), np.full(n0 * n1, 2.0)], axis=1)
    i, j = np.meshgrid(np.arange(n0 - 1), np.arange(n1 - 1), indexing="ij")
    a = (i * n1 + j).ravel()
    tris = np.concatenate([np.stack([a, a + n1, a + n1 + 1], axis=1), np.stack([a, a + n1 + 1, a + 1], axis=1)])
    return rest, tris.astype(np.int64)


def frames(rest, F, m, seed=0, h=0.05):
    rng = np.random.default_rng(seed)
    k = rng.normal(size=(m, 3))
    k *= (2 * np.pi / rng.uniform(1.0, 3.0, size=m) / np.linalg.norm(k, axis=1))[:, None]
    d = rng.normal(size=(m, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    modes = np.sin(rest @ k.T + rng.uniform(0, 6.28, size=m)[None]).T[:, :, None] * d[:, None, :]
    out = rest[None] + np.tensordot(rng.normal(size=(F, m)) * (0.08 / np.sqrt(m)), modes, axes=1)
    for f in range(F):
        out[f] += rng.normal(size=rest.shape) * (0.03 * h)
    return out


def normals(v, t):
    fn = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    n = np.zeros_like(v)
    for c in range(3):
        np.add.at(n, t[:, c], fn)
    return n / np.linalg.norm(n, axis=1)[:, None]


def leg(a):
    import torch
    from animsnapbases_amd import HipEngine, posComponents, posSnapshots
    rest, tris = grid(a.n0, a.n1)
    N = rest.shape[0]
    verts = frames(rest, a.frames, a.k + 8)
    param = types.SimpleNamespace(vertPos_bases_type="PCA", vertPos_numComponents=a.k, q_support="global",
                                  store_vertPos_PCA_sing_val=False, vertPos_smooth_min_dist=0.1, vertPos_smooth_max_dist=0.3,
                                  q_standarize=True, q_massWeight=False, q_orthogonal=False, vertPos_output_directory=".",
                                  name="time_onmesh")
    with contextlib.redirect_stdout(io.StringIO()):
        snaps = posSnapshots.from_arrays(verts, tris, "first", engine=HipEngine(0, stream=0))
        comp = posComponents(param, snaps)
        comp.compute_components_store_singvalues()
    out = {"leg": a.leg, "N": N, "F": a.frames, "r": a.k, "triangles": int(tris.shape[0])}
    if a.leg == "host":
        n0s, n1s = min(a.n0, 50), min(a.n1, 100)
        sub = (np.arange(n0s)[:, None] * a.n1 + np.arange(n1s)[None, :]).ravel()
        _, tsub = grid(n0s, n1s)
        t0 = time.perf_counter()
        T = snaps.snapTensor
        t1 = time.perf_counter()
        R = np.tensordot(comp.weigs[:, :a.k], comp.comps[:a.k][:, sub], axes=([1], [0]))
        X = T[:, sub] / snaps.pre_scale_factor + snaps.mean[None, sub]
        Xr = R / snaps.pre_scale_factor + snaps.mean[None, sub]
        denom = np.sqrt(3 * a.frames * sub.shape[0])
        acc_n, acc_a = np.zeros(sub.shape[0]), np.zeros(sub.shape[0])
        for f in range(a.frames):
            v, vr = X[f], Xr[f]
            acc_n += ((v - vr) ** 2).sum(axis=1) / (v ** 2).sum(axis=1) / denom
            n, nr = normals(v, tsub), normals(vr, tsub)
            acc_a += np.degrees(np.arccos(np.clip(np.einsum('ij,ij->i', n, nr), -1.0, 1.0)))
        t2 = time.perf_counter()
        out.update(subsample_vertices=int(sub.shape[0]), download_all_ms=(t1 - t0) * 1e3, host_subsample_ms=(t2 - t1) * 1e3,
                   host_extrapolated_ms=(t2 - t1) * 1e3 * N / sub.shape[0])
    else:
        want = a.leg == "normals"

        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            comp.on_mesh_accuracy(a.k, normals=want)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        run()
        ts = [run() for _ in range(3)]
        out.update(best_ms=min(ts), all_ms=ts, bytes_read_gb=24.0 * N * a.frames / 1e9, fma=3.0 * N * a.frames * a.k)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n0", type=int, default=250)
    ap.add_argument("--n1", type=int, default=400)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--leg", choices=["errors", "normals", "host"])
    ap.add_argument("--limit", type=int, default=420, help="seconds per leg")
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    for name in ("errors", "normals", "host"):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", name, "--n0", str(a.n0),
               "--n1", str(a.n1), "--frames", str(a.frames), "--k", str(a.k)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit("leg %s ended with status %d: nothing more is started" % (name, rc))


if __name__ == "__main__":
    main()
