"""Times the global step in a position subspace (csrc/asb_gsub.hip) against the explicit inverse and the slab
factor of the SAME build and process: device events around engine calls that drain the stream, best of 3.

    python tools/time_gsub.py [--tets 16667] [--frames 4032] [--ranks 16,64,256] [--m 64] [--json out.json]
    python tools/time_gsub.py --cloth 317 --frames 256        # the cloth grid of DESIGN.md 3.17: the inverse refuses it

Per solver -- "inverse", "slab" (target 256) and "subspace" with every r of ``--ranks`` (a random basis, orthonormalised by
``projections.subspace_basis``; the origin is the rest shape) -- in ms:
``setup_ms`` (asb_gstep_setup / asb_gslab_setup / asb_gsub_setup, host checks included), ``run_ms`` (asb_gstep_run), ``c_ms`` (the
constant c of a hyper step: a call of one iteration in "all" minus one iteration), ``operator_ms`` (asb_hyper_operator) and
``step_ms`` (one full time step of ``simulate_frames(hyper="touched")`` with ``--iterations`` iterations: (9 steps - 1 step) / 8
of the public call, whose host part -- the matrix is assembled on every call -- is tens of ms and cancels only in the
difference).  A solver that refuses the shape is listed with its message; every solver's figures also go to stderr as they come."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_cforces import best_of_3      # noqa: E402
from time_cproj import box      # noqa: E402
from time_gslab import cloth      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tets", type=int, default=16667)
    ap.add_argument("--cloth", type=int, default=0)
    ap.add_argument("--frames", type=int, default=4032)
    ap.add_argument("--ranks", default="16,64,256")
    ap.add_argument("--slab", type=int, default=256)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import torch
    from animsnapbases_amd import posSnapshots, projections, reduced
    ranks = [int(r) for r in a.ranks.split(",")]
    if a.cloth:
        kind, (rest, elems) = "tris_strain", cloth(a.cloth)
    else:
        kind, (rest, elems) = "tets_strain", box(a.tets)
    N, F, K, m = rest.shape[0], a.frames, a.iterations, a.m
    spec = dict(kind=kind, elements=elems, wi=1e3, rest_positions=rest, sigma_min=0.95, sigma_max=1.05)
    masses = 0.02 * (1.0 + 5.0 * np.random.default_rng(3).random(N))
    dt = 0.1
    res = dict(kind=kind, elements=int(elems.shape[0]), verts=N, frames=F, iterations=K, m=m, runs={})
    Amat = projections.global_matrix([(projections.build_setup(kind, elems, rest), 1e3)], N, masses, dt)
    comps = np.random.default_rng(7).standard_normal((max(ranks), N, 3))
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
    rows = term.St.shape[1]
    rng = np.random.default_rng(2)
    vecs = rng.standard_normal((m, rows, 3)) / np.sqrt(rows)
    Pt = rng.choice(rows, size=m, replace=False).astype(np.int64)
    p = term.setup.p
    basis = dict(components=vecs, interpol_alphas=Pt // p, Pt=Pt, interpol_alpha_ranges=np.arange(1, m + 1))
    op = reduced.reduced_operator(vecs, Pt // p, Pt, np.arange(1, m + 1), m, p, "deim_pod", n_elements=elems.shape[0])
    red_spec = dict(spec, basis=basis, num_components=m)

    def measure(tag, select, set_up):
        r = res["runs"].setdefault(tag, {})
        try:
            r["setup_ms"] = best_of_3(torch, set_up)
        except RuntimeError as e:
            r["refused"] = str(e)
            return
        eng.gstep_run(rhs.data_ptr(), F, out.data_ptr())
        r["run_ms"] = best_of_3(torch, lambda: eng.gstep_run(rhs.data_ptr(), F, out.data_ptr()))
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
        select()
        step = lambda T: snaps.simulate_frames([red_spec], dt, T, K, masses, hyper="touched")
        step(1)
        r["step_ms"] = (best_of_3(torch, lambda: step(9)) - best_of_3(torch, lambda: step(1))) / 8.0
        print(tag, json.dumps(r), file=sys.stderr, flush=True)

    measure("inverse", lambda: snaps.set_global_solver("inverse"), lambda: eng.gstep_setup(Amat))
    plan = projections.slab_plan(Amat, a.slab)
    measure("slab_%d" % a.slab, lambda: snaps.set_global_solver("slab", a.slab), lambda: eng.gslab_setup(Amat, plan))
    for r in ranks:
        Qt = projections.subspace_basis(comps, r)
        measure("subspace_%d" % r, lambda: snaps.set_global_solver("subspace", basis=comps, num_components=r, origin=rest),
                lambda: eng.gsub_setup(Amat, Qt, rest))
        res["runs"]["subspace_%d" % r]["held_bytes"] = int(8 * (2 * 3 * ((r + 15) // 16 * 16) * ((N + 31) // 32 * 32)))
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
