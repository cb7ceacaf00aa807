"""Times the hyper-reduced solver iterations at the shape of tools/time_pdsolve.py: 16 667 tetrahedra x 4 000 frames (N = 4 096),
m = 64 basis vectors, K = 10 iterations, device events around engine calls that drain the stream, best of 3
(csrc/asb_pdsolve.hip: asb_hyper_operator, asb_hyper_iterate) -- next to the reduced solve WITHOUT the operator from the same
build (asb_pdsolve_iterate with one reduced slot: k_cproj_em, k_rforce_coef, k_rforce_gemm, k_pd_add, k_pdsolve_gemm), which is
the path ``solve_frames`` took before ``hyper=`` existed.

    python tools/time_hyper.py [--tets 16667] [--frames 4000] [--m 64] [--iterations 10] [--json out.json]

What is timed: ``operator_ms`` one asb_hyper_operator (G = A^-1 S^T V); ``call_1_*`` / ``call_K1_*`` one asb_hyper_iterate of 1 and
of K + 1 iterations in "touched" and "all".  A call is c + (gathers) + iterations, and in "touched" its last iteration is a
full one, so the tool derives, as DIFFERENCES of call times and named as such:
  iteration_all_ms      = (call_K1_all - call_1_all) / K
  iteration_touched_ms  = (call_K1_touched - call_1_touched) / K
  c_ms                  = call_1_all - iteration_all_ms           (c, the memset of its buffer and the call's host work)
``baseline_iteration_ms``: asb_pdsolve_iterate(K) / K with the reduced slot.  The three public calls
``solve_frames(hyper=None | "touched" | "all")`` are timed once each end to end (host assembly included).

The basis is a random one with m distinct random sampled rows (``deim_pod``), as in tools/time_reduced_forces.py: the device
work depends on its shape only.  DESIGN.md section 3.15 records the figures."""
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
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import torch
    from animsnapbases_amd import posSnapshots, projections, reduced

    kind = "tets_strain"
    rest, tets = box(a.tets)
    N, F, K, m = rest.shape[0], a.frames, a.iterations, a.m
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
    snaps.global_solve_setup([spec], dt, masses)
    term, = snaps._plan([spec])
    setup, St, smin, smax = term.setup, term.St, term.sigma_min, term.sigma_max
    rows = St.shape[1]
    rng = np.random.default_rng(2)
    comps = rng.standard_normal((m, rows, 3)) / np.sqrt(rows)
    Pt = rng.choice(rows, size=m, replace=False).astype(np.int64)
    basis = dict(components=comps, interpol_alphas=Pt // 3, Pt=Pt, interpol_alpha_ranges=np.arange(1, m + 1))
    op = reduced.reduced_operator(comps, Pt // 3, Pt, np.arange(1, m + 1), m, 3, "deim_pod", n_elements=tets.shape[0])
    eng.rforce_operator(St, op.V)
    operator_ms = best_of_3(torch, eng.hyper_operator)
    sub = projections.subset_setup(setup, op.elements)
    touched, compact = projections.touched_setup(sub)
    diag, acc = masses / dt ** 2, np.zeros(3)
    out = torch.empty((F, N, 3), dtype=torch.float64, device=dev)

    def begin(su):
        eng.pdsolve_begin(0, 0, F, 1, None, False, 1.0, diag, 1, acc, 0)
        eng.cproj_setup(su)
        eng.rforce_solver(op.H, op.local_rows)
        eng.pdsolve_slot(smin, smax, None)
    res = dict(kind=kind, tets=int(tets.shape[0]), verts=N, frames=F, m=m, iterations=K, touched=int(touched.shape[0]),
               sampled_elements=int(op.elements.shape[0]), operator_ms=operator_ms)
    # the reduced solve without the operator: the baseline
    begin(sub)
    eng.pdsolve_iterate(1, 0, out.data_ptr())
    res["baseline_iteration_ms"] = best_of_3(torch, lambda: eng.pdsolve_iterate(K, 0, out.data_ptr())) / K
    for mode, su, tv in (("all", sub, None), ("touched", compact, touched)):
        begin(su)
        eng.hyper_iterate(1, tv, 0, out.data_ptr())
        res["call_1_%s_ms" % mode] = best_of_3(torch, lambda: eng.hyper_iterate(1, tv, 0, out.data_ptr()))
        res["call_K1_%s_ms" % mode] = best_of_3(torch, lambda: eng.hyper_iterate(K + 1, tv, 0, out.data_ptr()))
        res["iteration_%s_ms" % mode] = (res["call_K1_%s_ms" % mode] - res["call_1_%s_ms" % mode]) / K
    res["c_ms"] = res["call_1_all_ms"] - res["iteration_all_ms"]
    res["solve_K_touched_ms"] = res["call_1_touched_ms"] + (K - 1) * res["iteration_touched_ms"]
    res["solve_K_baseline_ms"] = K * res["baseline_iteration_ms"]
    # the public calls, end to end, once each (the first pays nothing the others do not: the inverse is held)
    red = dict(spec, basis=basis, num_components=m)
    for hyper in (None, "touched", "all"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        snaps.solve_frames([red], dt, K, masses, hyper=hyper)
        torch.cuda.synchronize()
        res["public_%s_s" % (hyper or "none")] = time.perf_counter() - t0
    res["flop_iteration_touched"] = 6.0 * F * touched.shape[0] * m
    res["flop_iteration_all"] = 6.0 * F * N * m
    res["flop_iteration_baseline"] = 6.0 * F * N * N + 6.0 * F * N * m
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
