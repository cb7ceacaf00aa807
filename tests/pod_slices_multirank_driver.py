"""Driver of tests/test_gpu_pod_slices_multirank.py::test_two_processes_gloo, started by ``torch.distributed.run`` with two
processes on device 0 and a gloo group: constProj_basis_type 'pod' on the pod_slices_p2 fixture (36 rows per rank: whole
constraints of 2); every rank saves the gathered basis to <out>/rank<r>.npz."""
import contextlib
import io
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out):
    import torch
    import torch.distributed as dist
    from animsnapbases_amd import constraintsComponents, nonlinearSnapshots
    from animsnapbases_amd.distributed import Comm

    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "pod_slices_p2.npz")))
    p, K = int(g["p"]), int(g["K"])
    param = types.SimpleNamespace(constProj_rest_shape="first", constProj_numFrames=0, constProj_p_size=p,
                                  constProj_massWeight=False, constProj_standarize=True, constProj_orthogonal=False,
                                  constProj_basis_type="pod", deim_desired_num_components=K, constProj_store_sing_val=False,
                                  constProj_output_directory=out, name="t", constProj_name="gloo",
                                  constProj_bases_interpolation_type="deim", constProj_snapshots_type="tris_strain")
    with contextlib.redirect_stdout(io.StringIO()):
        ns = nonlinearSnapshots(param, frames=g["frames"], comm=Comm())
        ns.config()
        ns.snapshots_prepare()
        cc = constraintsComponents(param, ns)
        cc.config()
        cc.compute_components_store_singvalues()
        comps = cc.comps
    os.makedirs(out, exist_ok=True)
    np.savez(os.path.join(out, "rank%d.npz" % rank), comps=comps)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
