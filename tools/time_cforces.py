"""Times posSnapshots.constraint_forces' device call (asb_cforce_run: k_cproj_em + k_st_apply per chunk of frames,
csrc/asb_cproj.hip) with device events, best of 3, at config 5's row count: 16 667 tetrahedra x 4 000 frames (N = 4 096) --
and the route it replaces on a 500-element x 50-frame subsample: constraint_projections, download of p, ``St @ p[f]`` per frame
with SciPy, extrapolated to the full shape.

    python tools/time_cforces.py [--tets 16667] [--frames 4000] [--kind tets_strain] [--chunk 0] [--json out.json]

The animation is synthesised on the device as in tools/time_cproj.py.  Between the events of the first leg lies the whole of
asb_cforce_run: the check and upload of the CSR of S^T (host work during which the device idles), then the kernels; the
kernels alone are what ``rocprofv3 --kernel-trace --stats`` of this script splits.  asb_cproj_run is timed the same way beside
it for the difference."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_cproj import box      # noqa: E402


def best_of_3(torch, fn):
    best = float("inf")
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tets", type=int, default=16667)
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--kind", default="tets_strain", choices=["tets_strain", "tets_deformation_gradient"])
    ap.add_argument("--chunk", type=int, default=0)
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
    snaps = posSnapshots.from_device(X.data_ptr(), F, N, "first", standarize=False, keepalive=X)
    spec = dict(kind=a.kind, elements=tets, wi=0.7, rest_positions=rest, sigma_min=0.95, sigma_max=1.05)
    out, nF = snaps.constraint_forces([spec], chunk_frames=a.chunk or None)         # warm-up; leaves the set-up on the device
    St = snaps.assembly_ST[a.kind]
    eng = snaps._engine
    rows = St.shape[1]
    force_ms = best_of_3(torch, lambda: eng.cforce_run(0, 0, F, 1, None, False, 1.0, 0.95, 1.05, St, False, a.chunk, out.data_ptr()))
    p = torch.empty((F, rows, 3), dtype=torch.float64, device=dev)
    eng.cproj_run(0, 0, F, 1, None, False, 1.0, 0.95, 1.05, p.data_ptr())
    proj_ms = best_of_3(torch, lambda: eng.cproj_run(0, 0, F, 1, None, False, 1.0, 0.95, 1.05, p.data_ptr()))
    res = dict(kind=a.kind, tets=int(tets.shape[0]), verts=N, frames=F, chunk_frames=a.chunk, nnz=int(St.nnz),
               cforce_ms=force_ms, cproj_ms=proj_ms, scratch_bytes_moved=2 * 8.0 * 3 * rows * F, out_bytes=8.0 * 3 * N * F,
               p_bytes=8.0 * 3 * rows * F)
    del p
    # the route this replaces, on 500 elements x 50 frames: projections on the device, download, one SciPy product per frame
    ne, nf = min(500, tets.shape[0]), min(50, F)
    sub = projections.assembly_ST(projections.build_setup(a.kind, tets[:ne], rest), N, 0.7)
    t0 = time.perf_counter()
    ps, _, _ = snaps.constraint_projections(a.kind, tets[:ne], rest_positions=rest, sigma_min=0.95, sigma_max=1.05, frame_end=nf)
    ph = ps.cpu().numpy()
    b = np.stack([sub @ ph[i] for i in range(nf)])
    host = time.perf_counter() - t0
    res["host_route_sub_ms"] = host * 1e3
    res["host_route_full_s_extrapolated"] = host * (tets.shape[0] / float(ne)) * (F / float(nf))
    chk, _ = snaps.constraint_forces([dict(spec, elements=tets[:ne])], frame_end=nf)
    res["max_abs_diff_sub"] = float(np.abs(chk.cpu().numpy() - b).max())
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
