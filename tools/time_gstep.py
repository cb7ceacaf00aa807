"""Times the global step at config 5's row count: 16 667 tetrahedra x 4 000 frames (N = 4 096), device events, best of 3 --
asb_gstep_setup once (host checks, dense fill, the N x N inverse, the residual), then asb_gstep_inertia and asb_gstep_run
(k_gstep_gemm, csrc/asb_gstep.hip) on the right-hand side asb_cforce_run left.

    python tools/time_gstep.py [--tets 16667] [--frames 4000] [--json out.json]

Cost model of the product, written before the first run: 2 * 3 * F' * N^2 = 4.0e11 flop, about 9 ms at the 45 TFLOP/s
k_interp_sweep reaches with the same f64 MFMA.  Traffic: rhs and out once each (2 x 393 MB), and the 134 MB of A^-1 once per
frame tile of 64 -- 63 tiles, 8.5 GB -- which has to come from L2 / Infinity Cache, not HBM: a block column of A^-1 (32
vertices, 1 MB) is shared by the 63 blocks of grid.y that run side by side.  The inertia term is elementwise: it reads the
tensor once or twice (393 / 786 MB) and reads and writes the right-hand side (786 MB), a fraction of a millisecond at HBM speed.

Every call returns after its stream has drained, so the events bracket the whole call as the host sees it: for the 9 ms
product that is the kernel; for asb_gstep_inertia it includes the host's finiteness check of ``diag`` and its upload, so that
figure is a call time, not a kernel time.

The animation is synthesised on the device as in tools/time_cforces.py; DESIGN.md section 3.13 records the figures."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_cforces import best_of_3      # noqa: E402
from time_cproj import box      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tets", type=int, default=16667)
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import torch
    from animsnapbases_amd import posSnapshots

    kind = "tets_strain"
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
    spec = dict(kind=kind, elements=tets, wi=1e3, rest_positions=rest, sigma_min=0.95, sigma_max=1.05)
    masses = 0.02 * (1.0 + 5.0 * np.random.default_rng(3).random(N))
    dt = 0.1
    eng = snaps._engine
    t0 = time.perf_counter()
    snaps.global_solve_setup([spec], dt, masses)                                     # (the first call also pays the allocations)
    setup_first_s = time.perf_counter() - t0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    eng.gstep_setup(snaps.global_matrix)
    e1.record()
    e1.synchronize()
    setup_ms = e0.elapsed_time(e1)
    b, nF = snaps.constraint_forces([spec])
    out = torch.empty_like(b)
    diag = masses / dt ** 2
    acc = np.zeros(3)
    inertia_ms = {}
    for mode in (0, 1):
        inertia_ms[mode] = best_of_3(torch, lambda: eng.gstep_inertia(0, 0, F, 1, None, False, 1.0, diag, mode, acc, b.data_ptr()))
    eng.gstep_run(b.data_ptr(), F, out.data_ptr())
    run_ms = best_of_3(torch, lambda: eng.gstep_run(b.data_ptr(), F, out.data_ptr()))
    flop = 6.0 * F * N * N
    res = dict(kind=kind, tets=int(tets.shape[0]), verts=N, frames=F, nnz=int(snaps.global_matrix.nnz),
               residual=float(snaps.global_solve_residual), setup_first_s=setup_first_s, setup_ms=setup_ms,
               inertia_zero_ms=inertia_ms[0], inertia_difference_ms=inertia_ms[1], run_ms=run_ms, run_flop=flop,
               run_tflops=flop / run_ms / 1e9, inverse_bytes=8.0 * N * N, tensor_bytes=8.0 * 3 * N * F)
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
