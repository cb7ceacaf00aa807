"""Times the global step's slab solver (csrc/asb_gslab.hip) against the explicit inverse of the SAME build:
device events around engine calls that drain the stream, best of 3.

    python tools/time_gslab.py [--tets 16667] [--frames 4000] [--targets 64,128,256,512,1536] [--m 64] [--json out.json]
    python tools/time_gslab.py --cloth 317 --frames 256 --targets 1536        # shape 2: a cloth grid the inverse refuses
    python tools/time_gslab.py --plan-only ...                                # the host plan and the flop counts, no device

Shape 1 (tools/time_pdsolve.py's: 16 667 tetrahedra, N = 4 096, F' = 4 000), under "inverse" and under every slab target:
``setup_ms`` (asb_gstep_setup / asb_gslab_setup, host checks included), ``run_ms`` (asb_gstep_run), ``iteration_ms`` (a full
asb_pdsolve_iterate iteration: (call of K + 1) - (call of 1) over K), ``c_ms`` (c = A^-1 ms of a hyper step: a call of one
iteration in "all" minus one iteration) and ``operator_ms`` (asb_hyper_operator).  Beside them the counts the expectation is
made of: ``flop_slab`` = 4 sum sp_k^2 W against ``flop_inverse`` = 2 N^2 W, W = 3 F' rounded up to 192, and ``z_bytes`` = 8 Npad W.
``gemm`` lists, for the padded slab sizes that occur, k_gslab_gemm and asb_gemm_nn on the same (sp x sp)(sp x W) product.
Shape 2 (``--cloth n``: n x n vertices, tris_strain, two triangles per cell): set-up, asb_gstep_run and the memory the factor
and the work matrices hold."""
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


def cloth(n):
    """n x n vertices on a unit-spaced grid, two triangles per cell."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    rest = np.stack([i.ravel() * 1.0, j.ravel() * 1.0, 0.05 * np.sin(0.3 * i.ravel()) * np.cos(0.2 * j.ravel())], axis=1)
    v = (i[:-1, :-1] * n + j[:-1, :-1]).ravel()
    tris = np.concatenate([np.stack([v, v + n, v + 1], axis=1), np.stack([v + 1, v + n, v + n + 1], axis=1)])
    return rest, tris.astype(np.int64)


def counts(plan, N, W):
    sp = (np.diff(plan.slab_ptr) + 15) // 16 * 16
    return dict(slabs=int(sp.size), sp_min=int(sp.min()), sp_max=int(sp.max()), sum_sp2=int((sp.astype(np.int64) ** 2).sum()),
                flop_slab=float(4.0 * (sp.astype(np.float64) ** 2).sum() * W), flop_inverse=float(2.0 * N * N * W),
                z_bytes=int(8 * sp.sum() * W))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tets", type=int, default=16667)
    ap.add_argument("--cloth", type=int, default=0)
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--targets", default="64,128,256,512,1536")
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--plan-only", action="store_true")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    from animsnapbases_amd import projections, reduced
    targets = [int(t) for t in a.targets.split(",")]
    if a.cloth:
        kind, (rest, elems) = "tris_strain", cloth(a.cloth)
    else:
        kind, (rest, elems) = "tets_strain", box(a.tets)
    N, F, K, m = rest.shape[0], a.frames, a.iterations, a.m
    W = (F + 63) // 64 * 64 * 3
    spec = dict(kind=kind, elements=elems, wi=1e3, rest_positions=rest, sigma_min=0.95, sigma_max=1.05)
    masses = 0.02 * (1.0 + 5.0 * np.random.default_rng(3).random(N))
    dt = 0.1
    res = dict(kind=kind, elements=int(elems.shape[0]), verts=N, frames=F, W=W, runs={})
    setup = projections.build_setup(kind, elems, rest)
    t0 = time.perf_counter()
    Amat = projections.global_matrix([(setup, 1e3)], N, masses, dt)
    res["host_matrix_s"] = time.perf_counter() - t0
    plans = {}
    for t in targets:
        t0 = time.perf_counter()
        plans[t] = projections.slab_plan(Amat, t)
        res["runs"]["slab_%d" % t] = dict(counts(plans[t], N, W), host_plan_s=time.perf_counter() - t0)
    if a.plan_only:
        print(json.dumps(res))
        return
    import torch
    from animsnapbases_amd import posSnapshots
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    R = torch.as_tensor(rest, device=dev)
    f = torch.arange(F, device=dev, dtype=torch.float64)
    X = (R[None] * (1.0 + 0.05 * torch.sin(0.011 * f))[:, None, None]
         + 0.002 * torch.randn((F, N, 3), generator=g, device=dev, dtype=torch.float64)).contiguous()
    X[0] = R
    snaps = posSnapshots.from_device(X.data_ptr(), F, N, "first", standarize=False, keepalive=X)
    eng = snaps._engine
    rhs = torch.randn((F, N, 3), generator=g, device=dev, dtype=torch.float64)
    out = torch.empty_like(rhs)
    diag, acc = masses / dt ** 2, np.zeros(3)
    term, = snaps._plan([spec])

    def measure(tag, set_up):
        r = res["runs"].setdefault(tag, {})
        r["setup_ms"] = best_of_3(torch, set_up)
        eng.gstep_run(rhs.data_ptr(), F, out.data_ptr())
        r["run_ms"] = best_of_3(torch, lambda: eng.gstep_run(rhs.data_ptr(), F, out.data_ptr()))
        if tag != "inverse":
            info = eng.gslab_info()
            r["factor_bytes"] = int(8 * info[3])
            r["work_bytes"] = int(8 * (info[2] + info[1]) * W)
        if a.cloth:
            return
        # a full iteration
        eng.pdsolve_begin(0, 0, F, 1, None, False, 1.0, diag, 1, acc, 0)
        eng.cproj_setup(term.setup)
        eng.pdsolve_slot(term.sigma_min, term.sigma_max, term.St)
        eng.pdsolve_iterate(1, 0, out.data_ptr())
        one = best_of_3(torch, lambda: eng.pdsolve_iterate(1, 0, out.data_ptr()))
        more = best_of_3(torch, lambda: eng.pdsolve_iterate(K + 1, 0, out.data_ptr()))
        r["iteration_ms"] = (more - one) / K
        # the hyper-reduced step: the operator and c
        rows = term.St.shape[1]
        rng = np.random.default_rng(2)
        comps = rng.standard_normal((m, rows, 3)) / np.sqrt(rows)
        Pt = rng.choice(rows, size=m, replace=False).astype(np.int64)
        op = reduced.reduced_operator(comps, Pt // 3, Pt, np.arange(1, m + 1), m, 3, "deim_pod", n_elements=elems.shape[0])
        eng.rforce_operator(term.St, op.V)
        eng.hyper_operator()
        r["operator_ms"] = best_of_3(torch, eng.hyper_operator)
        eng.pdsolve_begin(0, 0, F, 1, None, False, 1.0, diag, 1, acc, 0)
        eng.cproj_setup(projections.subset_setup(term.setup, op.elements))
        eng.rforce_solver(op.H, op.local_rows)
        eng.pdsolve_slot(term.sigma_min, term.sigma_max, None)
        eng.hyper_iterate(1, None, 0, out.data_ptr())
        one = best_of_3(torch, lambda: eng.hyper_iterate(1, None, 0, out.data_ptr()))
        more = best_of_3(torch, lambda: eng.hyper_iterate(K + 1, None, 0, out.data_ptr()))
        r["c_ms"] = one - (more - one) / K

    if not a.cloth:
        measure("inverse", lambda: eng.gstep_setup(Amat))
    else:
        try:
            eng.gstep_setup(Amat)
            res["inverse"] = "accepted"
        except RuntimeError as e:
            res["inverse"] = "refused: %s" % e
    for t in targets:
        measure("slab_%d" % t, lambda: eng.gslab_setup(Amat, plans[t]))
    sizes = sorted({16, 64, 128, 256, 512, 1024, 1536, 2048})
    res["gemm"] = {str(sp): dict(zip(("gslab_ms", "gemm_nn_ms"), eng.gslab_gemm_time(sp, W))) for sp in sizes}
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
