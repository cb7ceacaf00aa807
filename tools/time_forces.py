"""Times the start of a time step with external forces and the floor at the shape of tools/time_rollout.py: 16 667 tetrahedra x
4 000 frames (N = 4 096), frame_jump 1, one table row per step, the floor on; device events around engine calls that drain the
stream, best of 3 (csrc/asb_pdsolve.hip: asb_pdsolve_advance, asb_ext_set, asb_pdsolve_external).

    python tools/time_forces.py [--tets 16667] [--frames 4000] [--json out.json]

What is timed: ``advance_ms`` one asb_pdsolve_advance with nothing bound, followed by the engine's stream synchronisation (the call
itself does not wait) -- k_pd_advance, five 8-byte streams per entry; ``advance_ext_ms`` the same call with a per-step table and the
floor bound -- k_pd_advance_ext<2, true>, six streams; ``advance_const_ms`` / ``advance_floor_ms`` with a constant table and the
floor, and with the floor alone; ``external_ms`` one asb_pdsolve_external behind a fresh begin (the correction kernel, the upload of
diag and the call's own synchronisation); ``ext_set_ms`` the check and upload of the table.

Run from a checkout of the commit before this entry existed, the tool times ``advance_ms`` alone: that is the baseline DESIGN.md
section 3.22 records beside this build's figures."""
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
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import torch
    from animsnapbases_amd import posSnapshots

    rest, tets = box(a.tets)
    N, F = rest.shape[0], a.frames
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    R = torch.as_tensor(rest, device=dev)
    X = (R[None] * (1.0 + 0.1 * torch.sin(0.01 * torch.arange(F, device=dev, dtype=torch.float64))[:, None, None])
         + 0.002 * torch.randn((F, N, 3), generator=g, device=dev, dtype=torch.float64)).contiguous()
    snaps = posSnapshots.from_device(X.data_ptr(), F, N, "first", standarize=False, keepalive=X)
    spec = dict(kind="tets_strain", elements=tets, wi=1e3, rest_positions=rest, sigma_min=0.95, sigma_max=1.05)
    masses = 0.02 * (1.0 + 5.0 * np.random.default_rng(3).random(N))
    dt = 0.1
    eng = snaps._engine
    diag, acc = masses / dt ** 2, dt * dt * np.array([0.0, -9.81, 0.0])
    snaps.global_solve_setup([spec], dt, masses)
    res = dict(tets=int(tets.shape[0]), verts=N, frames=F, runs=3, state_tensor_bytes=24 * N * ((F + 63) // 64 * 64))

    def begin():
        eng.pdsolve_begin(0, 0, F, 1, None, False, 1.0, diag, 1, acc, 0)
        eng.pdsolve_carry(None)

    def advance():
        eng.pdsolve_advance()
        eng.sync()

    begin()
    advance()
    res["advance_ms"] = best_of_3(torch, advance)
    if hasattr(eng, "ext_set"):
        steps = 8
        table = 1e-3 * np.random.default_rng(4).standard_normal((F + steps, 3 * N))
        floor = (float(np.quantile(rest[:, 1], 0.3)), 1)
        res["table_bytes"] = int(table.nbytes)
        for tag, tb, fl in (("ext", table, floor), ("const", table[0], floor), ("floor", None, floor)):
            if tag == "ext":
                res["ext_set_ms"] = best_of_3(torch, lambda: eng.ext_set(tb, fl))
            else:
                eng.ext_set(tb, fl)
            best = float("inf")
            for _ in range(3):                      # (the binding is per begin: one timed call behind each)
                begin()
                best = min(best, _once(torch, lambda: eng.pdsolve_external(0)))
            if tag == "ext":
                res["external_ms"] = best
            advance()
            res["advance_%s_ms" % tag] = best_of_3(torch, advance)
        res["advance_ext_over_advance"] = res["advance_ext_ms"] / res["advance_ms"]
    res["advance_bytes"] = 5 * 24 * N * F
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


def _once(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


if __name__ == "__main__":
    main()
