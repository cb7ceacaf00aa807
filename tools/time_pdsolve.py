"""Times the solver iterations at the shape of tools/time_gstep.py: 16 667 tetrahedra x 4 000 frames (N = 4 096), device
events, best of 3 -- a 10-iteration ``solve_frames`` pass through the engine (asb_pdsolve_iterate: per iteration k_cproj_em,
k_st_apply, k_pd_add, k_pdsolve_gemm; csrc/asb_pdsolve.hip) next to its two parts alone on the same shape: ``global_solve``
(asb_gstep_run, k_gstep_gemm) and ``constraint_forces`` (asb_cforce_run, which re-uploads tables and S^T on every call).

    python tools/time_pdsolve.py [--tets 16667] [--frames 4000] [--iterations 10] [--json out.json]

Expectation, written before the first run: an iteration is the sum of the two parts plus the elementwise b += ms (three passes
over 393 MB, a fraction of a millisecond) minus the host work of asb_cforce_run; the vertex-major epilogue writes the same
393 MB as the frame-major one, in 512-byte runs instead of 768-byte ones.  An iteration noticeably above that sum is a finding
to explain.  The begin of a solve (inertia term, start state, uploads) and the slot registration are timed apart.

The animation is synthesised on the device as in tools/time_gstep.py; DESIGN.md section 3.14 records the figures."""
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
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import torch
    from animsnapbases_amd import posSnapshots

    kind = "tets_strain"
    rest, tets = box(a.tets)
    N, F, K = rest.shape[0], a.frames, a.iterations
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
    # the parts alone
    snaps.global_solve_setup([spec], dt, masses)
    term, = snaps._plan([spec])
    b = snaps._cforce_run([term], snaps._frames("train", 0, None, 1), None)
    out = torch.empty_like(b)
    setup, St, smin, smax = term.setup, term.St, term.sigma_min, term.sigma_max
    eng.cproj_setup(setup)
    cforce_ms = best_of_3(torch, lambda: eng.cforce_run(0, 0, F, 1, None, False, 1.0, smin, smax, St, False, 0, b.data_ptr()))
    eng.gstep_run(b.data_ptr(), F, out.data_ptr())
    solve_ms = best_of_3(torch, lambda: eng.gstep_run(b.data_ptr(), F, out.data_ptr()))
    # the solve: begin and slot once, then K iterations per timed call (each call continues the solve in progress)
    diag, acc = masses / dt ** 2, np.zeros(3)
    begin_ms = best_of_3(torch, lambda: eng.pdsolve_begin(0, 0, F, 1, None, False, 1.0, diag, 1, acc, 0))

    def slot():
        eng.pdsolve_begin(0, 0, F, 1, None, False, 1.0, diag, 1, acc, 0)
        eng.cproj_setup(setup)
        eng.pdsolve_slot(smin, smax, St)
    slot_ms = best_of_3(torch, slot) - begin_ms
    eng.pdsolve_iterate(1, 0, out.data_ptr())
    iterate_ms = best_of_3(torch, lambda: eng.pdsolve_iterate(K, 0, out.data_ptr()))
    history_ms = best_of_3(torch, lambda: eng.pdsolve_iterate(K, 0, out.data_ptr(), True))
    flop = 6.0 * F * N * N
    res = dict(kind=kind, tets=int(tets.shape[0]), verts=N, frames=F, iterations=K, cforce_ms=cforce_ms, global_solve_ms=solve_ms,
               parts_ms=cforce_ms + solve_ms, begin_ms=begin_ms, slot_ms=slot_ms, iterate_ms=iterate_ms,
               per_iteration_ms=iterate_ms / K, per_iteration_with_history_ms=history_ms / K,
               per_iteration_over_parts=iterate_ms / K / (cforce_ms + solve_ms), product_flop=flop,
               state_bytes=8.0 * 3 * N * (2 * F + (F + 63) // 64 * 64))
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
