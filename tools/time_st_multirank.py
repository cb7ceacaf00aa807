"""Halo and protocol overhead of 'pca_blocks_with_St' on several ranks, measured on ONE GPU: world 1 (the one-rank path)
against world 2 and 4 emulated by tests/thread_comm.py (every rank its own context on the same device, collectives through
the host).  The shape of tests/test_gpu_constraints_multirank.py's synthetic case: a 200 x 200 vertex triangle grid,
tri-strain constraints (p = 2, 79 202 triangles, 158 404 rows), F frames of a rank-20 animation, S^T assembled here;
natural and randomly permuted triangle numbering.  Reports h (halo rows) per rank and the wall time of the whole call.
These are not scaling numbers: the ranks share one device.

  python tools/time_st_multirank.py [--frames 64] [--reps 2]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    import torch
    from animsnapbases_amd import HipEngine
    from test_gpu_constraints_multirank import _param, _setup, _synthetic
    from thread_comm import run_ranks
    out = []
    for permuted in (False, True):
        frames, St, elems, p = _synthetic("_tris", permuted, a.frames, 20, 7 + a.frames)

        def one_run(world):
            def rank(r, comm):
                _, cc = _setup(_param(".", p, "pca_blocks_with_St", store=False, standarize=False), frames, St, elems,
                               engine=HipEngine(0, stream=0), comm=comm)
                torch.cuda.synchronize()
                if comm is not None:
                    comm.barrier()
                t0 = time.perf_counter()
                cc.compute_components_store_singvalues()
                torch.cuda.synchronize()
                return time.perf_counter() - t0, cc.st_halo_rows, cc.numComp
            with contextlib.redirect_stdout(io.StringIO()):
                if world == 1:
                    return [rank(0, None)]
                return run_ranks(world, rank)
        for world in (1, 2, 4):
            runs = [one_run(world) for _ in range(a.reps + 1)][1:]            # (the first call warms up)
            best = min(max(t for t, _, _ in res) for res in runs)
            out.append(dict(numbering="permuted" if permuted else "natural", world=world, seconds=round(best, 4),
                            halo_rows=runs[0][0][1], rows=int(frames.shape[1]), components=int(runs[0][0][2] * p)))
            print(json.dumps(out[-1]), flush=True)


if __name__ == "__main__":
    main()
