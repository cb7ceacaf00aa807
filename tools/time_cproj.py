"""Times asb_cproj_run (csrc/asb_cproj.hip) with device events, best of 3, at config 5's row count: 16 667 tetrahedra x
4 000 frames, and -- for scale -- the NumPy restatement (projections.project_host) on a 500-element x 50-frame subsample.

    python tools/time_cproj.py [--tets 16667] [--frames 4000] [--kind tets_strain] [--json out.json]

The animation is synthesised on the device (a box of tetrahedra that rotates, stretches and shears, plus noise) and adopted
through posSnapshots.from_device; only the kernel launches of asb_cproj_run lie between the events (the set-up upload is done
before).  Bytes: every input row once (3 N F doubles) plus the output (9 e F doubles), against 8 TB/s."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def box(n_tets, h=0.1):
    c = 1
    while 6 * c ** 3 < n_tets:
        c += 1
    n = c + 1
    vid = lambda i, j, k: (i * n + j) * n + k
    V = np.array([[i * h, j * h, k * h] for i in range(n) for j in range(n) for k in range(n)], dtype=np.float64)
    perms = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
    T = []
    for i in range(c):
        for j in range(c):
            for k in range(c):
                for pm in perms:
                    q = [i, j, k]
                    t = [vid(*q)]
                    for a in pm:
                        q[a] += 1
                        t.append(vid(*q))
                    T.append(t)
    return V, np.array(T[:n_tets], dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tets", type=int, default=16667)
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--kind", default="tets_strain", choices=["tets_strain", "tets_deformation_gradient"])
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import torch
    from animsnapbases_amd import posSnapshots, projections

    rest, tets = box(a.tets)
    N, F = rest.shape[0], a.frames
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    R = torch.as_tensor(rest, device=dev)
    f = torch.arange(F, device=dev, dtype=torch.float64)
    A = torch.eye(3, device=dev, dtype=torch.float64).repeat(F, 1, 1)
    A[:, 0, 0] += 0.3 * torch.sin(0.011 * f)
    A[:, 1, 1] -= 0.25 * torch.sin(0.007 * f + 1)
    A[:, 0, 1] += 0.2 * torch.sin(0.009 * f)
    A[:, 2, 1] += 0.1 * torch.cos(0.005 * f)
    X = (torch.einsum("fij,nj->fni", A, R) + 0.002 * torch.randn((F, N, 3), generator=g, device=dev, dtype=torch.float64)).contiguous()
    X[0] = R
    world = X[:50].cpu().numpy()
    snaps = posSnapshots.from_device(X.data_ptr(), F, N, "first", standarize=False, keepalive=X)
    out, nF, rows = snaps.constraint_projections(a.kind, tets, rest_positions=rest, sigma_min=0.95, sigma_max=1.05)      # warm-up
    eng = snaps._engine
    best = float("inf")
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.cproj_run(0, 0, F, 1, None, False, 1.0, 0.95, 1.05, out.data_ptr())
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    nbytes = 8.0 * (3 * N * F + 3 * rows * F)
    res = dict(kind=a.kind, tets=int(tets.shape[0]), verts=N, frames=F, device_ms=best, bytes=nbytes,
               tb_per_s=nbytes / (best * 1e-3) / 1e12, frac_of_8tbs=nbytes / (best * 1e-3) / 8e12)
    # scale: the host restatement on 500 elements x 50 frames, and its figure extrapolated to the full shape
    sub = projections.build_setup(a.kind, tets[:500], rest)
    t0 = time.perf_counter()
    ref = projections.project_host(sub, world, 0.95, 1.05)
    host = time.perf_counter() - t0
    res["host_sub_ms"] = host * 1e3
    res["host_full_s_extrapolated"] = host * (tets.shape[0] / 500.0) * (F / 50.0)
    res["max_abs_diff_sub"] = float(np.abs(out[:50, :sub.rows].cpu().numpy() - ref).max())
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
