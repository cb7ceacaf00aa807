"""CPU: the small-mesh cases of tests/geodesic_cases.py and the model of tests/geodesic_model.py that the GPU tests of
tests/test_gpu_geodesic_small.py compare the device with -- the case table, the model against the host SuperLU oracle, what the
float64 model loses against the longdouble one (the yardstick of the GPU tolerances, and that it stays below their ceilings),
the predicted Jacobi sweep counts of the sparse mode, and two properties of the host set-up that nothing else asserts directly:
bfs_slabs returns a block-tridiagonal numbering, mesh_aggregates a partition."""
import numpy as np
import pytest
from scipy import sparse

import geodesic_cases as gc
import geodesic_model as gm
from animsnapbases_amd.geodesic import bfs_slabs, mesh_aggregates
from oracle import asb_oracle as orc

EPS = 2.0 ** -52
MARGIN, FLOOR = 100.0, 50 * EPS
CEIL_DIRECT, CEIL_SPARSE = 1e-9, 1e-8           # tests/test_gpu_geodesic_pcg.py's acceptance levels
TOL = 1e-13                                     # the PCG tolerance of the sparse mode
SLAB_TARGETS = (1, 40, 100, 1536)
LD = np.longdouble


def test_case_table():
    print("\n    case     n      np    nb  nblk  triangles  valences")
    for name in gc.CASES:
        V, T = gc.mesh(name)
        n, np_, nb = gc.expected(name)
        got = gc.padded(V.shape[0])
        val = np.bincount(np.concatenate([T[:, [0, 1]], T[:, [1, 2]], T[:, [2, 0]]]).ravel(), minlength=V.shape[0]) // 2
        print("    %-8s %-6d %-5d %-3d %-5d %-10d %d .. %d" % (name, V.shape[0], got[0], got[1], got[2], T.shape[0], val.min(), val.max()))
        assert V.shape[0] == n and got[:2] == (np_, nb), (name, V.shape[0], got)
        assert T.min() == 0 and T.max() == n - 1 and np.unique(T).shape[0] == n        # every vertex is used
        assert sparse.csgraph.connected_components(gc.operators(name)[0])[0] == 1
    assert gc.expected("tiny")[0] % 16 and gc.padded(20)[2] == 5
    assert 593 <= gc.expected("n600")[0] <= 608 and gc.expected("n600")[0] % 16
    assert (gc.expected("stride")[0] + 3) // 4 > 1024
    assert {gc.expected(c)[0] for c in ("n127", "n128", "n129", "n255", "n257", "n511", "n512")} == {127, 128, 129, 255, 257, 511, 512}


def test_sources_hold_the_ends_and_one_duplicate():
    for n in (20, 129, 600):
        for k in (15, 16, 17, 33, 48, 49, 64):
            s = gc.sources(n, k)
            assert s.shape == (k,) and 0 in s and n - 1 in s and s.min() >= 0 and s.max() < n
            if n - 2 >= k - 3:
                assert np.unique(s).shape[0] == k - 1
            assert set(s.tolist()) <= set(gc.sources(n, 64).tolist())
        assert gc.sources(n, 1).tolist() == [n - 1]


def test_band_cholesky_is_a_cholesky():
    rng = np.random.default_rng(0)
    for n, bw in ((1, 0), (7, 0), (9, 2), (30, 29), (40, 5)):
        A = rng.normal(size=(n, n))
        A = A @ A.T + n * np.eye(n)
        i, j = np.indices((n, n))
        A[abs(i - j) > bw] = 0
        A += 2 * np.abs(A).sum(axis=1).max() * np.eye(n)
        B = rng.normal(size=(n, 3))
        for dtype in (np.float64, LD):
            W = gm.band_cholesky(gm.band_from_sparse(sparse.csr_matrix(A), dtype))
            assert W.shape[1] == bw + 1
            x = gm.band_solve(W, B.astype(dtype))
            assert x.dtype == dtype and gm.deviation(A.astype(dtype) @ x, B)[0] < 1e-14
        assert gm.deviation(gm.cholesky_inverse(A.astype(LD)), np.linalg.inv(A))[0] < 1e-13


@pytest.mark.parametrize("name", gc.CASES)
def test_model_vs_oracle_and_float64_yardstick(name):
    V, T = gc.mesh(name)
    ref = gm.reference(name)
    oracle = orc.Geodesics(V, T)
    pick = ref["src"][[0, ref["src"].shape[0] // 2, -1]]
    for s in pick:
        fro, mx = gm.deviation(oracle(int(s)), gm.rows(ref, "hi", [s])[0])
        print("%s source %d: oracle (SuperLU) vs longdouble model %.2e / %.2e" % (name, s, fro, mx))
        assert fro < 1e-9 and mx < 1e-9
    assert ref["hi"].dtype == LD and ref["lo"].dtype == np.float64
    assert (ref["hi"].min(axis=1) == 0).all() and (ref["hi"][np.arange(ref["src"].shape[0]), ref["src"]] < 0.05 * ref["hi"].max()).all()
    worst = [0.0, 0.0]
    for q in range(ref["src"].shape[0]):
        fro, mx = gm.deviation(ref["lo"][q], ref["hi"][q])
        worst = [max(worst[0], fro), max(worst[1], mx)]
    kappa = ref["kappa"]
    assert (ref["kappa_heat"] is not None) == (V.shape[0] < 512) and kappa >= ref["kappa_poisson"]
    b_direct = max(FLOOR, MARGIN * max(worst))
    b_sparse = max(b_direct, kappa * TOL)
    print("%s: float64 vs longdouble model %.2e / %.2e per field; cond(A_heat) %s, cond(-L) %.1f; bound direct %.2e, sparse %.2e"
          % (name, worst[0], worst[1], ref["kappa_heat"], ref["kappa_poisson"], b_direct, b_sparse))
    assert b_direct <= CEIL_DIRECT, "the reference alone is above the ceiling of the dense and slab modes"
    assert b_sparse <= CEIL_SPARSE, "the reference alone is above the ceiling of the sparse mode"


def test_grounded_poisson_form_equals_the_gauge_form(monkeypatch):
    """the longdouble model's form of step 4 above DENSE_LIMIT vertices, against the literal one: equal but for the rows of the
    float64 L not summing to zero exactly (<= 8 terms of eps |L_ii| each), which the solve amplifies by cond(-L) at the most"""
    ops = gc.operators("n255")
    src = [0, 100, 254]
    lit = gm.HeatModel(*ops, dtype=LD)
    monkeypatch.setattr(gm, "DENSE_LIMIT", 100)
    gr = gm.HeatModel(*ops, dtype=LD)
    assert gr.grounded and not lit.grounded
    fro, mx = gm.deviation(gr.fields(src), lit.fields(src))
    print("grounded vs gauge-fixed Poisson step in longdouble: %.2e / %.2e" % (fro, mx))
    bound = 8 * EPS * gm.condition_numbers(ops[0], ops[1], want_heat=False)[1]
    assert fro < bound and mx < bound, bound


def test_predicted_heat_sweeps():
    print("\n    case     omega   rho        predicted sweeps")
    for name in gc.SPARSE_CG_CASES + gc.SPARSE_SWEEP_CASES:
        omega, rho, sweeps = gc.jacobi_sweeps(gc.operators(name)[0])
        print("    %-8s %-7.3f %-10.6f %.0f%s" % (name, omega, rho, sweeps, "" if name in gc.SPARSE_SWEEP_CASES else "  (n < 512: PCG, no sweeps)"))
        if name in gc.SPARSE_SWEEP_CASES:
            assert sweeps <= gc.SWEEP_LIMIT, (name, sweeps)


def slab_layout(name, target):
    """(order, ptr, slab of the grounded last vertex, that slab's size)"""
    order, ptr = bfs_slabs(gc.operators(name)[0], target)
    return order, ptr, ptr.shape[0] - 2, int(ptr[-1] - ptr[-2])


@pytest.mark.parametrize("name", gc.CASES)
def test_bfs_slabs_make_a_block_tridiagonal_numbering(name):
    A = gc.operators(name)[0]
    n = A.shape[0]
    for target in SLAB_TARGETS:
        order, ptr = bfs_slabs(A, target)
        assert sorted(order.tolist()) == list(range(n)), (name, target, "not a permutation")
        assert ptr[0] == 0 and ptr[-1] == n and (np.diff(ptr) > 0).all(), (name, target, ptr)
        P = A[order][:, order].tocoo()
        slab_of = np.repeat(np.arange(ptr.shape[0] - 1), np.diff(ptr))
        far = np.abs(slab_of[P.row] - slab_of[P.col]) > 1
        assert not far.any(), (name, target, "entries outside the block tridiagonal", int(far.sum()))
        print("%s target %d: %d slabs, sizes %d .. %d, last %d" % (name, target, ptr.shape[0] - 1, np.diff(ptr).min(), np.diff(ptr).max(),
                                                                    ptr[-1] - ptr[-2]))
    assert bfs_slabs(A, 1)[1][1] == 1                      # every level a slab: the first is the start vertex alone


def test_slab_cases_of_the_gpu_module():
    counts = {(name, target): bfs_slabs(gc.operators(name)[0], target)[1].shape[0] - 1 for name, target in gc.SLAB_CASES}
    print(counts)
    assert counts == gc.SLAB_COUNTS
    assert counts[("tiny", 1536)] == 1 and counts[("stride", 1536)] == 3
    ragged = [(name, target) for name, target in gc.SLAB_CASES if slab_layout(name, target)[3] % 16]
    assert ragged, "no case grounds a vertex inside a padded slab"


@pytest.mark.parametrize("name", gc.CASES)
def test_mesh_aggregates_partition(name):
    A = gc.operators(name)[0]
    agg, nc = mesh_aggregates(A)
    assert agg.shape == (A.shape[0],) and agg.min() == 0 and agg.max() == nc - 1
    assert np.unique(agg).shape[0] == nc, "an unused label"
    print("%s: %d aggregates of %d .. %d vertices" % (name, nc, np.bincount(agg).min(), np.bincount(agg).max()))
    if name == "n600":
        assert nc % 16, "the coarse level of n600 is to need padding"


def test_support_weights_and_slab_gemm_models():
    phi = np.array([0.0, 0.1, 0.25, 0.3, 0.7])
    s = gm.support_weights(phi, 1, 3, 0.1, 0.3)
    assert s.tolist() == [1.0, 1.0 - (0.25 - 0.1) / (0.3 - 0.1), 0.0]
    rng = np.random.default_rng(0)
    A, Z, out = rng.normal(size=(16, 32)), rng.normal(size=(32, 64)), rng.normal(size=(16, 64))
    out[:, 5] = np.nan
    r = gm.slab_gemm(A, Z, out, 1.0, 0.0, 2)
    assert np.isfinite(r[:, :32]).all() and gm.deviation(r[:, :32], A @ Z[:, :32])[0] < 1e-15
    assert np.array_equal(r[:, 32:], out[:, 32:].astype(LD))
    r = gm.slab_gemm(A, Z, out, -1.0, 1.0, 9)
    assert gm.deviation(np.delete(r, 5, axis=1), np.delete(out - A @ Z, 5, axis=1))[0] < 1e-15
