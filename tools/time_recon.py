"""Timing of the reconstruction-error sweeps at config 4 (100 000 vertices x 2 000 frames, K = 128, global support, U[-1,1)
frames from a seed): the train sweep 1..128 step 1 (one read of X) and a held-out animation of F' frames (upload + Gram
products + factor + sweep, and the sweep alone).  Host clock around calls that end in a device synchronise.

  python tools/time_recon.py [--n 100000] [--frames 2000] [--k 128] [--test-frames 2000] [--reps 5]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--test-frames", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from animsnapbases_amd import posComponents, posSnapshots
    rng = np.random.default_rng(0)
    verts = rng.uniform(-1, 1, size=(a.frames, a.n, 3))
    test = rng.uniform(-1, 1, size=(a.test_frames, a.n, 3))
    param = types.SimpleNamespace(vertPos_bases_type="PCA", vertPos_numComponents=a.k, q_support="global",
                                  store_vertPos_PCA_sing_val=False, vertPos_smooth_min_dist=0.1, vertPos_smooth_max_dist=0.3,
                                  q_standarize=True, q_massWeight=False, q_orthogonal=False, vertPos_output_directory=".",
                                  name="time_recon")
    with contextlib.redirect_stdout(io.StringIO()):
        snaps = posSnapshots.from_arrays(verts, None, "first", test_verts=test)
        comp = posComponents(param, snaps)
        comp.compute_components_store_singvalues()
    eng = snaps._engine
    ks = np.arange(1, a.k + 1)

    def best(fn):
        fn()                                  # warm-up (code objects, buffers)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return min(ts), float(np.median(ts))

    out = {"N": a.n, "F": a.frames, "K": a.k, "F_test": a.test_frames}
    out["train_sweep_ms"] = best(lambda: eng.recon_sweep(0, ks))
    out["test_convergence_ms"] = best(lambda: comp.test_convergence(1, a.k, 1))
    out["heldout_total_ms"] = best(lambda: comp.reconstruction_errors(1, a.k, 1, "test"))
    out["heldout_sweep_ms"] = best(lambda: eng.recon_sweep(1, ks))
    # f64 work of one sweep: per element and k one FMA; per element and sweep point a subtract, a square-add and a max
    elems = 3.0 * a.n * a.frames
    out["train_sweep_gflop"] = elems * (2 * a.k + 4 * len(ks)) / 1e9
    out["bytes_read_gb"] = elems * 8 / 1e9
    print(json.dumps(out))


if __name__ == "__main__":
    main()
