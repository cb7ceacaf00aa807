"""Times the reduced constraint term beside the full one at config 5's row count: 16 667 tetrahedra x 4 000 frames (N = 4 096),
device events, best of 3 -- asb_cforce_run (the full S^T p, tools/time_cforces.py) against asb_rforce_run with m basis vectors
(k_cproj_em on the sampled elements, k_rforce_coef, k_rforce_gemm; csrc/asb_rforce.hip), and once each the set-up
asb_rforce_operator (S^T V on the device) and asb_force_diff.

    python tools/time_reduced_forces.py [--tets 16667] [--frames 4000] [--m 64] [--json out.json]

The animation is synthesised on the device as in tools/time_cforces.py.  The basis is a random one with m distinct random
sampled rows (``deim_pod``): the device work depends on its shape only, the errors it gives mean nothing."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_cforces import best_of_3      # noqa: E402
from time_cproj import box      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tets", type=int, default=16667)
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import torch
    from animsnapbases_amd import posSnapshots, projections, reduced

    kind = "tets_strain"
    rest, tets = box(a.tets)
    N, F, m = rest.shape[0], a.frames, a.m
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
    spec = dict(kind=kind, elements=tets, wi=0.7, rest_positions=rest, sigma_min=0.95, sigma_max=1.05)
    full, nF = snaps.constraint_forces([spec])                                       # warm-up; leaves S^T
    St = snaps.assembly_ST[kind]
    eng = snaps._engine
    rows = St.shape[1]
    args = (0, 0, F, 1, None, False, 1.0, 0.95, 1.05)
    setup = projections.build_setup(kind, tets, rest)
    eng.cproj_setup(setup)
    full_ms = best_of_3(torch, lambda: eng.cforce_run(*args, St, False, 0, full.data_ptr()))

    rng = np.random.default_rng(2)
    comps = rng.standard_normal((m, rows, 3)) / np.sqrt(rows)
    Pt = rng.choice(rows, size=m, replace=False).astype(np.int64)
    op = reduced.reduced_operator(comps, Pt // 3, Pt, np.arange(1, m + 1), m, 3, "deim_pod", n_elements=tets.shape[0])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    eng.rforce_operator(St, op.V)
    e1.record()
    e1.synchronize()
    operator_ms = e0.elapsed_time(e1)
    eng.cproj_setup(projections.subset_setup(setup, op.elements))
    eng.rforce_solver(op.H, op.local_rows)
    red = torch.empty_like(full)
    eng.rforce_run(*args, False, red.data_ptr())
    red_ms = best_of_3(torch, lambda: eng.rforce_run(*args, False, red.data_ptr()))
    diff_ms = best_of_3(torch, lambda: eng.force_diff(full.data_ptr(), red.data_ptr(), F, N))
    res = dict(kind=kind, tets=int(tets.shape[0]), verts=N, frames=F, m=m, sampled_elements=int(op.elements.shape[0]),
               nnz=int(St.nnz), cond=[float(c) for c in op.cond], cforce_ms=full_ms, rforce_ms=red_ms,
               rforce_operator_ms=operator_ms, force_diff_ms=diff_ms, gemm_flop=6.0 * N * m * F, out_bytes=8.0 * 3 * N * F)
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
