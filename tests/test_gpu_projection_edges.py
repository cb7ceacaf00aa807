"""GPU (-m gpu): the projection kernels and the projection mode at the shapes where they branch.

* The column projection out = X . W / col_scale (asb_test_project_columns) through the 16-column kernel and through
  launch_wide at every tile count 1..8, against exact integer arithmetic (bit for bit) and against the float64 product
  with an elementwise rounding bound; F around the 16-frame chunks, the 1008-frame sweep and the 2048-frame limit of the
  co-resident panel kernel; row counts below one row group and many groups per block; columns beyond ncols must stay
  untouched.
* The ASB_WIDE_VARIANT forms of the four-tile kernel, each in a child process (the variant is read once per process).
* Single-rank projection mode (both device modes) and the multi-rank driver on one GPU against the oracle for F on both
  sides of 2048, with the statistics saying which side each run took; more than four sub-panels per read of X.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import align_signs, relerr
from oracle import asb_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(np.float64).eps
COOP_MAX_F = 2048          # frames of a row the co-resident panel kernel holds (asb.h: asb_panel_coop_possible)

# (F, N, ncols, path): path 0 = 16 columns per pass, path 1 = launch_wide with ceil(ncols / 16) tiles.  Every edge value of
# F and N, every tile count 1..8 and every ragged column count appear at least once (test_cases_cover_the_edges).
CASES = [
    (1, 21, 17, 1), (15, 5, 33, 1), (16, 21, 63, 1), (17, 1, 64, 1), (1008, 21, 65, 1), (1009, 5, 90, 1),
    (1024, 21, 100, 1), (1025, 21, 127, 1), (2000, 21, 128, 1), (2033, 5, 64, 1), (2048, 21, 64, 1), (2049, 21, 15, 1),
    (4000, 21, 64, 1), (4000, 5, 128, 1), (2000, 1, 1, 1), (257, 30000, 64, 1), (257, 30000, 128, 1), (257, 30000, 17, 1),
    (1, 5, 1, 0), (17, 21, 33, 0), (1008, 21, 16, 0), (1009, 21, 17, 0), (2000, 5, 15, 0), (2049, 21, 40, 0),
    (4000, 1, 16, 0), (257, 30000, 33, 0),
]
K0, LD_EXTRA = 3, 5         # the columns start at k0 > 0 of a wider W (ldw > k0 + ncols)


def _tiles(ncols):
    return (ncols + 15) // 16


def _run_columns(e, W, ncols, scale, path):
    out = np.full((ncols + 3, 3 * e.n_loc), np.nan)                 # three sentinel columns behind the ncols written ones
    e.test_project_columns(W, K0, ncols, out, col_scale=scale, path=path)
    assert np.isnan(out[ncols:]).all(), "the kernel wrote beyond its %d columns" % ncols
    return out[:ncols]


def check_case(F, N, ncols, path, seed=0):
    """Integer-exact and float-bounded checks of one shape (also the body of the variant children)."""
    from animsnapbases_amd import HipEngine
    rng = np.random.default_rng(seed + 7919 * F + 31 * N + ncols)
    ldw = K0 + ncols + LD_EXTRA
    e = HipEngine(0)
    try:
        # (1) integers: |x|, |w| <= 1000, so every product and every partial sum of <= 4000 of them is an integer below
        # 2^53 -- exact in f64 in any order (not in f32) -- and the scales are powers of two: the expected result is exact
        Xi = rng.integers(-1000, 1001, size=(F, N, 3))
        Wi = rng.integers(-1000, 1001, size=(F, ldw))
        scale = 2.0 ** rng.integers(-3, 4, size=ldw) if (F + ncols) % 2 else None
        e.upload(Xi.astype(np.float64), 0, N)
        got = _run_columns(e, Wi.astype(np.float64), ncols, scale, path)
        Xm = Xi.reshape(F, 3 * N)                                   # device row 3 v + d = column 3 v + d of the frame-major X
        Wc = Wi[:, K0:K0 + ncols]
        if F * N * ncols <= 2e7:
            ref = (Wc.T @ Xm).astype(np.float64)                    # int64 product
        else:                                                       # same numbers: exact in f64, see above
            ref = Wc.T.astype(np.float64) @ Xm.astype(np.float64)
        if scale is not None:
            ref = ref / scale[K0:K0 + ncols, None]
        bad = np.argwhere(got != ref)
        assert bad.size == 0, ("integer product not exact", F, N, ncols, path, bad[:5].tolist(), got[tuple(bad[0])],
                               ref[tuple(bad[0])])
        # (2) uniform floats against the float64 product: |out - ref| <= 4 F eps (|W|^T |X|) elementwise
        Xf = rng.uniform(-1, 1, size=(F, N, 3))
        Wf = rng.uniform(-1, 1, size=(F, ldw))
        sf = rng.uniform(0.5, 2.0, size=ldw)
        e.upload(Xf, 0, N)
        got = _run_columns(e, Wf, ncols, sf, path)
        Xm, Wc, sc = Xf.reshape(F, 3 * N), Wf[:, K0:K0 + ncols], sf[K0:K0 + ncols, None]
        ref = (Wc.T @ Xm) / sc
        bound = 4 * F * EPS * ((np.abs(Wc).T @ np.abs(Xm)) / sc) + 2 * EPS * np.abs(ref)
        over = np.abs(got - ref) - bound
        assert (over <= 0).all(), ("float product outside the rounding bound", F, N, ncols, path,
                                   np.unravel_index(np.argmax(over), over.shape), float(over.max()))
    finally:
        e.close()


@pytest.mark.parametrize("F,N,ncols,path", CASES)
def test_project_columns_exact(F, N, ncols, path):
    check_case(F, N, ncols, path)


def test_cases_cover_the_edges():
    """The case table itself: every edge value and every tile count at least once."""
    assert {c[0] for c in CASES} >= {1, 15, 16, 17, 1008, 1009, 1024, 1025, 2000, 2033, 2048, 2049, 4000}
    assert {c[1] for c in CASES} >= {1, 5, 21, 30000}
    assert {_tiles(c[2]) for c in CASES if c[3] == 1} == set(range(1, 9))
    assert {c[2] for c in CASES} >= {1, 15, 17, 33, 63, 64, 65, 127, 128}
    assert {c[3] for c in CASES} == {0, 1}


# the four-tile kernel's variants (csrc/asb_project.hip: launch_l2w); the variant is a function-static getenv
VARIANT_CASES = [(17, 21, 64), (2000, 5, 63), (2049, 21, 64), (257, 30000, 64), (1, 1, 49)]


def _child_variant():
    for F, N, ncols in VARIANT_CASES:
        check_case(F, N, ncols, 1, seed=11)
    print("variant %s: %d cases OK" % (os.environ.get("ASB_WIDE_VARIANT"), len(VARIANT_CASES)))


def _child(body, env_over, timeout):
    env = dict(os.environ, **env_over)
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_projection_edges as t; t.%s()" % (ROOT, HERE, body)
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=timeout)
    err = p.stderr.decode(errors="replace")
    assert p.returncode == 0, (p.returncode, err[-4000:])
    return p.stdout.decode()


@pytest.mark.parametrize("variant", [45, 47, 51, 52])
def test_wide_variants_exact(variant):
    out = _child("_child_variant", {"ASB_WIDE_VARIANT": str(variant)}, timeout=300)
    assert "cases OK" in out, out


def _data(kind, F, N, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.uniform(-1, 1, size=(F, N, 3))
    return np.tensordot(rng.normal(size=(F, 8)) * (0.7 ** np.arange(8)), rng.normal(size=(8, N, 3)), (1, 0)) \
        + 1e-4 * rng.normal(size=(F, N, 3))


def _assert_matches_oracle(out, ref):
    assert out["idx"].tolist() == ref["idx"].tolist()
    comps, weigs = align_signs(out["comps"], out["weigs"], ref["comps"])
    assert relerr(comps, ref["comps"]) < 1e-8
    assert relerr(weigs, ref["weigs"]) < 1e-8
    assert relerr(out["sigma"], ref["measures"][:, 1]) < 1e-9


@pytest.mark.parametrize("kind", ["random", "lowrank"])
@pytest.mark.parametrize("F", [2033, 2048, 2049, 4000])
def test_project_mode_across_frame_limit(F, kind):
    """Single rank, N above the candidate capacity: both device modes equal the oracle on either side of F = 2048, and the
    projection mode ran the co-resident panel kernel exactly when F <= 2048."""
    from animsnapbases_amd import HipEngine
    N, K = 3000, 40
    X = _data(kind, F, N, seed=F)
    ref = orc.extract_k_components(X, K)
    for mode in (0, 1):
        e = HipEngine(0)
        try:
            e.upload(X, 0, N)
            e.deflate_begin(K, False, mode)
            if mode == 1:
                assert N > e.panel_capacity()
                assert e.panel_coop_possible() == (F <= COOP_MAX_F)
            e.run_global(0, K)
            out = e.results()
            st = e.deflate_stats() if mode == 1 else None
        finally:
            e.close()
        _assert_matches_oracle(out, ref)
        if mode == 1:
            assert st["panels"] >= 1, st
            if F <= COOP_MAX_F:
                assert st["coop_launches"] >= 1, st
            else:
                assert st["coop_launches"] == 0 and st["guessed_panels"] == 0, st


@pytest.mark.parametrize("F", [2049, 4000])
def test_multirank_project_above_frame_limit(F):
    """The multi-rank driver (two ranks on one GPU) with F > 2048: the co-resident kernel cannot run, so the driver must
    stay on the per-panel path (it used to ask the library for the one-launch read, which refuses above 2048)."""
    import contextlib
    import io
    import types
    from animsnapbases_amd import HipEngine, posComponents, posSnapshots
    from thread_comm import run_ranks
    world, N, K = 2, 3000, 40
    verts = np.random.default_rng(F).uniform(-1, 1, size=(F, N, 3))
    param = types.SimpleNamespace(vertPos_bases_type="PCA", q_standarize=True, q_massWeight=False, q_orthogonal=False,
                                  q_support="global", vertPos_numComponents=K, store_vertPos_PCA_sing_val=False,
                                  vertPos_smooth_min_dist=0.1, vertPos_smooth_max_dist=0.25, vertPos_rest_shape="first",
                                  name="t", vertPos_output_directory=".")

    def rank_fn(rank, comm):
        with contextlib.redirect_stdout(io.StringIO()):
            snaps = posSnapshots.from_arrays(verts, None, "first", standarize=True, massWeight=False,
                                             engine=HipEngine(0, stream=0), comm=comm)
            comp = posComponents(param, snaps)
            comp.deflate_mode = "project"
            comp.compute_components_store_singvalues()
        return comp.selected_vertices.copy(), comp.comps.copy(), comp.weigs.copy()

    outs = run_ranks(world, rank_fn)
    pre = orc.prepare_snapshots(verts, "first", True)
    ref = orc.extract_k_components(pre["snapTensor"], K)
    for idx, comps, weigs in outs:
        assert idx.tolist() == ref["idx"].tolist()
        comps, weigs = align_signs(comps, weigs, ref["comps"])
        assert relerr(comps, ref["comps"]) < 1e-8 and relerr(weigs, ref["weigs"]) < 1e-8


SUB8 = dict(F=2000, N=3000, K=128)


def _child_sub_panels8():
    from animsnapbases_amd import HipEngine
    F, N, K = SUB8["F"], SUB8["N"], SUB8["K"]
    X = _data("random", F, N, seed=5)
    e = HipEngine(0)
    try:
        e.upload(X, 0, N)
        e.deflate_begin(K, False, 1)
        e.run_global(0, K)
        out = e.results()
        st = e.deflate_stats()
    finally:
        e.close()
    _assert_matches_oracle(out, orc.extract_k_components(X, K))
    print("STATS " + json.dumps(st))


def test_eight_sub_panels_per_read():
    """ASB_SUB_PANELS=8 ASB_SUB_FIRST=8: reads of X with up to eight sub-panels (tiles 5..8 of the multi-tile kernel inside a
    real run) equal the oracle, and at least one read committed more than 64 components."""
    out = _child("_child_sub_panels8", {"ASB_SUB_PANELS": "8", "ASB_SUB_FIRST": "8"}, timeout=600)
    st = json.loads([l for l in out.splitlines() if l.startswith("STATS ")][-1][6:])
    assert st["coop_launches"] >= 1, st
    assert st["max_read_kept"] > 64, st
