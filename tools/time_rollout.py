"""Times one time step of a roll-out at the shape of tools/time_hyper.py: 16 667 tetrahedra x 4 000 frames (N = 4 096), m = 64
basis vectors, K = 10 iterations per step, device events around engine calls that drain the stream, best of 3
(csrc/asb_pdsolve.hip: asb_pdsolve_carry, asb_pdsolve_advance, asb_pdsolve_positions).

    python tools/time_rollout.py [--tets 16667] [--frames 4000] [--m 64] [--iterations 10] [--pins 0] [--json out.json]

What is timed: ``advance_ms`` one asb_pdsolve_advance followed by the engine's stream synchronisation (the call itself does not
wait); ``positions_ms`` one asb_pdsolve_positions; ``carry_ms`` one asb_pdsolve_carry from the frames; ``step_full_ms`` one
asb_pdsolve_iterate(K) with the kind's full term followed by an advance; ``step_touched_ms`` one asb_hyper_iterate(K) on the
touched rows followed by an advance; ``iterate_full_ms`` / ``iterate_touched_ms`` the same calls without the advance.  The two
public calls ``simulate_frames(num_steps=3, hyper=None | "touched")`` are timed once each end to end (host assembly included).

The basis is a random one with m distinct random sampled rows (``deim_pod``), as in tools/time_hyper.py: the device work
depends on its shape only.  DESIGN.md section 3.16 records the figures.

``--pins P`` (P > 0): P positional constraints with a per-pin shift are bound to every timed solve (asb_pins_set once,
asb_pdsolve_pins behind every begin; their weights are in the matrix), so every advance also launches the pin kernel; ``pin_term_ms``
is one asb_pins_term into a frame-major tensor.  DESIGN.md section 3.19 records those figures next to the run without pins."""
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
    ap.add_argument("--pins", type=int, default=0)
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
    diag, acc = masses / dt ** 2, np.zeros(3)
    pins = None
    if a.pins > 0:                                  # spread over the mesh, stiff, each on a path of its own
        v = np.linspace(0, N - 1, a.pins).astype(np.int64)
        shift = 0.01 * np.sin(0.01 * np.arange(F + 256)[:, None, None] + np.arange(a.pins)[None, :, None] + np.arange(3)[None, None, :])
        pins = dict(vertices=v, wi=1e3, positions=rest[v], shift=shift)
        snaps.global_solve_setup([spec], dt, masses, pins=pins)
        rec = snaps._pins("time_rollout", pins)
        eng.pins_set(rec.vertices, rec.wi, rec.p0, rec.shift)
    else:
        snaps.global_solve_setup([spec], dt, masses)

    def begin():
        eng.pdsolve_begin(0, 0, F, 1, None, False, 1.0, diag, 1, acc, 0)
        if pins is not None:
            eng.pdsolve_pins(0)
    term, = snaps._plan([spec])
    setup, St, smin, smax = term.setup, term.St, term.sigma_min, term.sigma_max
    rows = St.shape[1]
    rng = np.random.default_rng(2)
    comps = rng.standard_normal((m, rows, 3)) / np.sqrt(rows)
    Pt = rng.choice(rows, size=m, replace=False).astype(np.int64)
    basis = dict(components=comps, interpol_alphas=Pt // 3, Pt=Pt, interpol_alpha_ranges=np.arange(1, m + 1))
    op = reduced.reduced_operator(comps, Pt // 3, Pt, np.arange(1, m + 1), m, 3, "deim_pod", n_elements=tets.shape[0])
    touched, compact = projections.touched_setup(projections.subset_setup(setup, op.elements))
    out = torch.empty((F, N, 3), dtype=torch.float64, device=dev)
    res = dict(kind=kind, tets=int(tets.shape[0]), verts=N, frames=F, m=m, iterations=K, touched=int(touched.shape[0]), runs=3, pins=a.pins,
               state_tensor_bytes=24 * N * ((F + 63) // 64 * 64))

    def advance():
        eng.pdsolve_advance()
        eng.sync()

    # the full path
    begin()
    res["carry_ms"] = best_of_3(torch, lambda: eng.pdsolve_carry(None))
    eng.cproj_setup(setup)
    eng.pdsolve_slot(smin, smax, St)
    advance()
    res["advance_ms"] = best_of_3(torch, advance)
    res["positions_ms"] = best_of_3(torch, lambda: eng.pdsolve_positions(out.data_ptr()))
    # (a fresh state for the iterations: repeated advances alone walk away from the animation)
    begin()
    eng.pdsolve_carry(None)
    eng.cproj_setup(setup)
    eng.pdsolve_slot(smin, smax, St)
    eng.pdsolve_iterate(1, 0, None)
    res["iterate_full_ms"] = best_of_3(torch, lambda: eng.pdsolve_iterate(K, 0, None))
    res["step_full_ms"] = best_of_3(torch, lambda: (eng.pdsolve_iterate(K, 0, None), advance()))
    # the hyper-reduced path on the touched rows
    eng.rforce_operator(St, op.V)
    eng.hyper_operator()
    begin()
    eng.pdsolve_carry(None)
    eng.cproj_setup(compact)
    eng.rforce_solver(op.H, op.local_rows)
    eng.pdsolve_slot(smin, smax, None)
    eng.hyper_iterate(1, touched, 0, None)
    res["iterate_touched_ms"] = best_of_3(torch, lambda: eng.hyper_iterate(K, touched, 0, None))
    res["step_touched_ms"] = best_of_3(torch, lambda: (eng.hyper_iterate(K, touched, 0, None), advance()))
    red = dict(spec, basis=basis, num_components=m)
    kw = {} if pins is None else dict(pins=pins)
    if pins is not None:
        res["pin_term_ms"] = best_of_3(torch, lambda: eng.pins_term(0, F, 1, 0, True, out.data_ptr()))
    for hyper in (None, "touched"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        snaps.simulate_frames([red], dt, 3, K, masses, hyper=hyper, **kw)
        torch.cuda.synchronize()
        res["public_3_steps_%s_s" % (hyper or "none")] = time.perf_counter() - t0
    res["advance_bytes"] = 5 * 24 * N * F
    res["advance_TBps"] = res["advance_bytes"] / (res["advance_ms"] * 1e-3) / 1e12
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
