"""Timing of the interpolation-error sweeps of constraint bases at config-5 shape (50 000 constraint rows x 4 000 frames,
K = 256, pod_vectorized + post-processing + DEIM, seeded low-rank frames plus noise; F' = 4 000 held-out frames): the train
and test sweeps r = 1..256 (constraintsComponents.interpolation_errors) and, for comparison, the existing path for ONE r
(geom_constructed + the reference's three host metrics).  Host clock around calls that end in a device synchronise.

  python tools/time_interp.py [--ep 50000] [--frames 4000] [--k 256] [--test-frames 4000] [--reps 3]
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
    ap.add_argument("--ep", type=int, default=50000)
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--test-frames", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    from animsnapbases_amd import constraintsComponents, nonlinearSnapshots
    rng = np.random.default_rng(5)
    Ft = a.frames + a.test_frames
    modes = rng.normal(size=(a.k + 20, a.ep * 3))
    coef = rng.normal(size=(Ft, a.k + 20)) * (0.97 ** np.arange(a.k + 20))[None]
    allf = (coef @ modes).reshape(Ft, a.ep, 3)
    allf += 1e-6 * rng.standard_normal(size=allf.shape, dtype=np.float32)
    del modes
    param = types.SimpleNamespace(constProj_rest_shape="first", constProj_numFrames=0, constProj_p_size=1,
                                  constProj_massWeight=False, constProj_standarize=True, constProj_orthogonal=False,
                                  constProj_basis_type="pod_vectorized", deim_desired_num_components=a.k,
                                  constProj_store_sing_val=False, constProj_output_directory=".", name="time_interp",
                                  constProj_name="c5", constProj_bases_interpolation_type="deim",
                                  constProj_snapshots_type="tris_strain")
    with contextlib.redirect_stdout(io.StringIO()):
        ns = nonlinearSnapshots(param, frames=allf[:a.frames], test_frames=allf[a.frames:])
        ns.config()
        ns.snapshots_prepare()
        cc = constraintsComponents(param, ns)
        cc.config()
        cc.compute_components_store_singvalues()
        cc.post_process_components()
        cc.deim()
    del allf
    rs = list(range(1, a.k + 1))

    def best(fn, reps):
        fn()                                  # warm-up (code objects, buffers)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return min(ts), float(np.median(ts))

    out = {"ep": a.ep, "F": a.frames, "K": a.k, "F_test": a.test_frames}
    out["train_sweep_ms"] = best(lambda: cc.interpolation_errors(rs, "train"), a.reps)
    out["test_sweep_ms"] = best(lambda: cc.interpolation_errors(rs, "test"), a.reps)
    # f64 work of one sweep: the reconstruction products 2 ep F rp per coordinate, the coefficients 2 rp npt F per coordinate
    npt = [int(cc.geom_alpha_ranges[r - 1]) for r in rs]
    flop = sum(6.0 * a.ep * a.frames * r + 6.0 * r * n * a.frames for r, n in zip(rs, npt))
    out["train_sweep_tflop"] = flop / 1e12
    out["train_tflops"] = flop / 1e12 / (out["train_sweep_ms"][0] / 1e3)
    out["test_tflops"] = flop * a.test_frames / a.frames / 1e12 / (out["test_sweep_ms"][0] / 1e3)

    def old_path():
        f = ns.snapTensor
        rec = cc.geom_constructed(a.k, "train")
        cc.frobenius_error(f, rec), cc.max_pointwise_error(f, rec), cc.relative_error_per_component(f, rec)
    t0 = time.perf_counter()
    old_path()                                # (first call includes the one download of snapTensor)
    out["geom_constructed_r256_first_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    old_path()
    out["geom_constructed_r256_ms"] = (time.perf_counter() - t0) * 1e3
    out["geom_constructed_x256_extrapolated_s"] = out["geom_constructed_r256_ms"] * a.k / 1e3
    print(json.dumps(out))


if __name__ == "__main__":
    main()
