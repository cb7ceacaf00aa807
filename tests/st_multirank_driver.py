"""Driver of tests/test_gpu_constraints_multirank.py::test_two_processes_gloo, started by ``torch.distributed.run`` with two
processes on device 0 and a gloo group: 'pca_blocks_with_St' and then the position-space geometric interpolation on the
with_st_p2 fixture; every rank saves what it got to <out>/rank<r>.npz."""
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
    from scipy import sparse
    from animsnapbases_amd import constraintsComponents, nonlinearSnapshots
    from animsnapbases_amd.distributed import Comm

    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "with_st_p2.npz")))
    p, K = int(g["p"]), int(g["pos_K"])
    St = sparse.csr_matrix((g["St_data"], g["St_indices"], g["St_indptr"]), shape=tuple(g["St_shape"]))

    def run(basis, K_):
        param = types.SimpleNamespace(constProj_rest_shape="first", constProj_numFrames=0, constProj_p_size=p,
                                      constProj_massWeight=False, constProj_standarize=True, constProj_orthogonal=False,
                                      constProj_basis_type=basis, deim_desired_num_components=K_, constProj_store_sing_val=False,
                                      constProj_support="global", constProj_output_directory=out, name="st", constProj_name="gloo",
                                      constProj_bases_interpolation_type="geom", constProj_snapshots_type="tris_strain",
                                      constProj_element_type="_tris", bases_R_tol=1e-8, geom_ele_per_vert=2)
        ns = nonlinearSnapshots(param, frames=g["frames"], comm=Comm())
        ns.config()
        ns.tris = g["tris"]
        ns.snapshots_prepare()
        cc = constraintsComponents(param, ns)
        cc.config()
        cc.St = St
        cc.compute_components_store_singvalues()
        return cc

    res = {}
    with contextlib.redirect_stdout(io.StringIO()):
        cc = run("pca_blocks_with_St", 0)
        res.update(verts=cc.largeDeforPoints, blocks=cc.largeDeforBlocks, comps=cc.comps, weigs=cc.weigs,
                   meas=cc.measures_at_largeDeforVerts)
        cc = run("pca_blocks", K)           # (70 rows per rank: whole constraints of 2)
        cc.geom_block_form_utilizing_differential_operator(True)
        res.update(g_verts=cc.geom_interpol_verts, g_alpha=cc.geom_alpha, g_Pt=cc.geom_Pt, g_ranges=cc.geom_alpha_ranges)
    os.makedirs(out, exist_ok=True)
    np.savez(os.path.join(out, "rank%d.npz" % rank), **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
