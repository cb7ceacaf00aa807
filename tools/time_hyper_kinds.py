"""Times the hyper-reduced solver iterations with TWO reduced kinds in one solve (``set_reduced_kinds``) at the
shape of tools/time_hyper.py with a second kind: 16 667 tetrahedra x 4 000 frames (N = 4 096), ``tets_strain`` on the
tetrahedra and ``edge_spring`` on their edges, m = 64 random basis vectors and 64 sampled elements each, K = 10 iterations,
device events around engine calls that drain the stream, best of 3.

    python tools/time_hyper_kinds.py [--tets 16667] [--frames 4000] [--m 64] [--iterations 10] [--json out.json]

What is timed.  ``operator_bank<b>_ms``: one asb_hyper_operator per bank.  ``call_1_*`` / ``call_K1_*``: one asb_hyper_iterate
of 1 and of K + 1 iterations in "touched" (the union of the two kinds' touched vertices, ``touched``) and "all", with both
kinds' slots (``two_*``) and, from the same build and the same context, with the tetrahedra alone (``one_*``: what
tools/time_hyper.py times; the single-kind yardstick of the parent commit is that tool run there).  As in tools/time_hyper.py the
tool derives, as DIFFERENCES of call times and named as such:
  *_iteration_all_ms      = (call_K1_all - call_1_all) / K
  *_iteration_touched_ms  = (call_K1_touched - call_1_touched) / K
  *_c_ms                  = call_1_all - iteration_all_ms
``two_plain_iteration_ms``: asb_pdsolve_iterate(K) / K with the two reduced slots and no operator A^-1 S^T V (the N^2 product
stays in the loop).  Launches per touched iteration and chunk: 2 S + 1 for S kinds (k_cproj_em and k_rforce_coef per kind, one
k_hyper_apply), 5 against 3.

The bases are random ones with m distinct random sampled rows (``deim_pod``): the device work depends on their shape only."""
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
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import torch
    from animsnapbases_amd import posSnapshots, projections, reduced

    rest, tets = box(a.tets)
    edges = np.unique(np.sort(np.concatenate([tets[:, [i, j]] for i in range(4) for j in range(i + 1, 4)]), axis=1), axis=0)
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
    snaps.set_reduced_kinds(2)
    specs = [dict(kind="tets_strain", elements=tets, wi=1e3, rest_positions=rest, sigma_min=0.95, sigma_max=1.05),
             dict(kind="edge_spring", elements=edges, wi=1e2, rest_positions=rest)]
    masses = 0.02 * (1.0 + 5.0 * np.random.default_rng(3).random(N))
    dt = 0.1
    eng = snaps._engine
    snaps.global_solve_setup(specs, dt, masses)
    terms = snaps._plan(specs)
    rng = np.random.default_rng(2)
    ops, bases, subs = [], [], []
    for t in terms:
        rows, p = t.St.shape[1], t.setup.p
        comps = rng.standard_normal((m, rows, 3)) / np.sqrt(rows)
        Pt = rng.choice(rows, size=m, replace=False).astype(np.int64)
        bases.append(dict(components=comps, interpol_alphas=Pt // p, Pt=Pt, interpol_alpha_ranges=np.arange(1, m + 1)))
        ops.append(reduced.reduced_operator(comps, Pt // p, Pt, np.arange(1, m + 1), m, p, "deim_pod", n_elements=t.setup.n_elem))
        subs.append(projections.subset_setup(t.setup, ops[-1].elements))
    res = dict(kinds=[t.kind for t in terms], tets=int(tets.shape[0]), edges=int(edges.shape[0]), verts=N, frames=F, m=m, iterations=K)
    for b, (t, op) in enumerate(zip(terms, ops)):
        eng.rforce_bank(b)
        eng.rforce_operator(t.St, op.V)
        res["operator_bank%d_ms" % b] = best_of_3(torch, eng.hyper_operator)
    eng.rforce_bank(0)
    diag, acc = masses / dt ** 2, np.zeros(3)
    out = torch.empty((F, N, 3), dtype=torch.float64, device=dev)

    def begin(which, setups):
        eng.pdsolve_begin(0, 0, F, 1, None, False, 1.0, diag, 1, acc, 0)
        for b in which:
            eng.rforce_bank(b)
            eng.cproj_setup(setups[b])
            eng.rforce_solver(ops[b].H, ops[b].local_rows)
            eng.pdsolve_slot(terms[b].sigma_min, terms[b].sigma_max, None)
        eng.rforce_bank(0)
    for tag, which in (("one", (0,)), ("two", (0, 1))):
        union = projections.touched_union([subs[b] for b in which])
        res[tag + "_touched"] = int(union.shape[0])
        compact = {b: projections.touched_setup(subs[b], into=union)[1] for b in which}
        begin(which, subs)
        eng.pdsolve_iterate(1, 0, out.data_ptr())
        res[tag + "_plain_iteration_ms"] = best_of_3(torch, lambda: eng.pdsolve_iterate(K, 0, out.data_ptr())) / K
        for mode, su, tv in (("all", subs, None), ("touched", compact, union)):
            begin(which, su)
            eng.hyper_iterate(1, tv, 0, out.data_ptr())
            c1 = best_of_3(torch, lambda: eng.hyper_iterate(1, tv, 0, out.data_ptr()))
            cK = best_of_3(torch, lambda: eng.hyper_iterate(K + 1, tv, 0, out.data_ptr()))
            res["%s_call_1_%s_ms" % (tag, mode)], res["%s_call_K1_%s_ms" % (tag, mode)] = c1, cK
            res["%s_iteration_%s_ms" % (tag, mode)] = (cK - c1) / K
        res[tag + "_c_ms"] = res[tag + "_call_1_all_ms"] - res[tag + "_iteration_all_ms"]
    res["touched_two_over_one"] = res["two_iteration_touched_ms"] / res["one_iteration_touched_ms"]
    res["all_two_over_one"] = res["two_iteration_all_ms"] / res["one_iteration_all_ms"]
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
