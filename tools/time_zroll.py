"""Times a roll-out whose state lives in z (csrc/asb_zroll.hip) against the parent's path of the SAME build, process
and session, ``simulate_frames(hyper="touched")`` under ``set_global_solver("subspace")``: device events around public calls that
drain the stream, best of 3 after a warm-up.

    python tools/time_zroll.py [--tets 16667] [--frames 4032] [--ranks 16,64,256] [--m 64] [--json out.json]
    python tools/time_zroll.py --cloth 317 --frames 256        # the cloth grid of DESIGN.md 3.17

The shapes, the random basis, the reduced kind and the method are those of tools/time_gsub.py.  Per r, in ms: ``parent_step_ms`` and
``zstep_ms`` (one time step of ``--iterations`` iterations: (9 steps - 1 step) / 8 of the public call, whose host part -- the matrix is
assembled on every call, 50 - 400 ms -- cancels in the difference only to its own spread; ``*_step32_ms``: (33 - 1) / 32 of the same),
``zstep_engine_ms`` ((65 steps - 1 step) / 64 of asb_zroll_steps alone from a freshly begun roll-out: no host part at all), ``operator_ms`` (asb_zroll_operator), ``begin_ms`` (asb_zroll_begin: T, kappa,
the touched rows and the projection of the start, the per-call set-up) and ``call1_ms`` (the whole public call of one step, host
part included).  Every r's figures also go to stderr as they come."""
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
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import torch
    from animsnapbases_amd import posSnapshots, projections
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
    term, = snaps._plan([spec])
    rows = term.St.shape[1]
    rng = np.random.default_rng(2)
    vecs = rng.standard_normal((m, rows, 3)) / np.sqrt(rows)
    Pt = rng.choice(rows, size=m, replace=False).astype(np.int64)
    p = term.setup.p
    basis = dict(components=vecs, interpol_alphas=Pt // p, Pt=Pt, interpol_alpha_ranges=np.arange(1, m + 1))
    red_spec = dict(spec, basis=basis, num_components=m)
    diag, acc = masses / dt ** 2, np.zeros(3)
    def engine_steps(T):
        """asb_zroll_steps alone, T steps from a freshly begun roll-out (the public call of one step, untimed, begins it): best of 3."""
        best = float("inf")
        for _ in range(3):
            snaps.simulate_subspace([red_spec], dt, 1, K, masses)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.zroll_steps(T, K)
            e1.record()
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1))
        return best

    for r in ranks:
        out = res["runs"].setdefault("r_%d" % r, {})
        snaps.set_global_solver("subspace", basis=comps, num_components=r, origin=rest)
        parent = lambda T: snaps.simulate_frames([red_spec], dt, T, K, masses, hyper="touched")
        zroll = lambda T: snaps.simulate_subspace([red_spec], dt, T, K, masses)
        parent(1)
        p1, p9, p33 = (best_of_3(torch, lambda T=T: parent(T)) for T in (1, 9, 33))
        out["parent_step_ms"], out["parent_step32_ms"] = (p9 - p1) / 8.0, (p33 - p1) / 32.0
        zroll(1)
        z1, z9, z33 = (best_of_3(torch, lambda T=T: zroll(T)) for T in (1, 9, 33))
        out["zstep_ms"], out["zstep32_ms"], out["call1_ms"] = (z9 - z1) / 8.0, (z33 - z1) / 32.0, z1
        out["zstep_engine_ms"] = (engine_steps(65) - engine_steps(1)) / 64.0
        out["operator_ms"] = best_of_3(torch, eng.zroll_operator)
        touched = projections.touched_setup(projections.subset_setup(term.setup, np.unique(Pt // p)))[0]
        begin = lambda: eng.zroll_begin(0, 0, F, 1, None, False, snaps.pre_scale_factor, diag, 1, acc, touched)
        begin()
        out["begin_ms"] = best_of_3(torch, begin)
        out["touched"] = int(touched.shape[0])
        print("r = %d" % r, json.dumps(out), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
