"""Writes tests/golden/pdsolve_reduced_combined.npz (CPU only, NumPy and the package's host routines; never imported by a test).

    python tools/gen_golden_multireduced.py

What the tests of several reduced kinds in one solve (tests/multireduced_cases.py) need stored:

  edge_<key>   the constraint basis of ``edge_spring`` on the 18-vertex ``combined`` mesh, the four keys of
               ``reduced.BASIS_KEYS``: ``hyper_cases.chain_basis`` of ``project_host``'s output over the 130 frames.  Stored, so
               that LAPACK's free signs and pivot ties cannot move it under the amps below.
  dg_<key>     the same for ``tets_deformation_gradient`` on the fixture's tetrahedra (interpolation elements = Pt // 3).
  amp_<me>_<mt>_<mode>_<K>
               the amplification tests/pdsolve_cases.py defines, measured ON THE HOST MODEL of tests/multireduced_cases.py with
               the edges reduced to me in {1, 3, 4, 17} and the tetrahedra (tests/golden/reduced_forces_tets_deim.npz) to mt in
               {1, 17} components, per velocity mode and K in {1, 3, 10}.
  amp_mixed_<mode>_<K>
               the same for ``mixed_case``: edges reduced (m = 4), tets_strain plain, tets_deformation_gradient reduced (m = 4).

Every amp is held to ``AMP_CAP`` and every normal matrix to ``COND_CAP`` here; the union sizes and the distance of the
both-reduced solve from the full and the tets-only-reduced solves (the non-vacuity margin of the GPU test) are printed."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multireduced_cases as mc      # noqa: E402
import pdsolve_cases as pc      # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def main():
    a = mc.combined_case(load)
    mixed = mc.mixed_case(load)
    F, N = a["frames"].shape[:2]
    arrays = {"edge_" + k: np.asarray(a["bases"][0][k]) for k in mc.BASIS_KEYS}
    arrays.update({"dg_" + k: np.asarray(mixed["bases"][2][k]) for k in mc.BASIS_KEYS})
    full = {mode: mc.model(a, range(F), mode, (10,))[10] for mode in pc.MODES}
    worst_cond = worst_amp = 0.0
    for me in mc.EDGE_MS:
        for mt in mc.TET_MS:
            ops = {0: a["op"](0, me), 1: a["op"](1, mt)}
            worst_cond = max(worst_cond, float(max(o.cond.max() for o in ops.values())))
            union, _, own = mc.sampled(a, ops)
            for mode in pc.MODES:
                amp = mc.measure_amp(a, mode, reduced=ops)
                both = mc.model(a, range(F), mode, (10,), reduced=ops)[10]
                tets_only = mc.model(a, range(F), mode, (10,), reduced={1: ops[1]})[10]
                for K in pc.KS:
                    assert amp[K] <= pc.AMP_CAP, (me, mt, mode, K, amp[K])
                    arrays[mc.amp_key(me, mt, mode, K)] = np.float64(amp[K])
                    worst_amp = max(worst_amp, amp[K])
                print("me = %2d mt = %2d %-10s: amp %s, N_t %d | %d -> %d of %d, |both - full| %.3g, |both - tets only| %.3g"
                      % (me, mt, mode, " ".join("%.3g" % amp[K] for K in pc.KS), own[0].shape[0], own[1].shape[0], union.shape[0], N,
                         np.abs(both - full[mode]).max(), np.abs(both - tets_only).max()))
    ops = {0: mixed["op"](0, mc.MIXED_MS[0]), 2: mixed["op"](2, mc.MIXED_MS[1])}
    worst_cond = max(worst_cond, float(max(o.cond.max() for o in ops.values())))
    for mode in pc.MODES:
        amp = mc.measure_amp(mixed, mode, reduced=ops)
        for K in pc.KS:
            assert amp[K] <= pc.AMP_CAP, ("mixed", mode, K, amp[K])
            arrays["amp_mixed_%s_%d" % (mode, K)] = np.float64(amp[K])
            worst_amp = max(worst_amp, amp[K])
        print("mixed %-10s: amp %s" % (mode, " ".join("%.3g" % amp[K] for K in pc.KS)))
    assert worst_cond <= mc.COND_CAP, worst_cond
    print("largest cond %.3g (cap %.3g), largest amp %.3g (cap %.3g)" % (worst_cond, mc.COND_CAP, worst_amp, pc.AMP_CAP))
    path = os.path.join(GOLDEN, "pdsolve_reduced_combined.npz")
    np.savez(path, edge_ms=np.array(mc.EDGE_MS, dtype=np.int64), tet_ms=np.array(mc.TET_MS, dtype=np.int64),
             mixed_ms=np.array(mc.MIXED_MS, dtype=np.int64), **arrays)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print("%s %.1f KB" % (os.path.basename(path), size / 1024.0))


if __name__ == "__main__":
    main()
