"""GPU (-m gpu): constraintsComponents.interpolation_errors / store_convergence_tests (asb_interp.hip) -- the convergence test of
run_geom_tests (generate_figures/nl_reduction_tests.py:117-225) on the device, against the reference's fixtures and against
geom_constructed (constraintsComponents.py:489-521) plus the reference's three metrics (:524-556) on the host."""
import contextlib
import csv
import io
import os
import types

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu


def _cparam(K, tmp, kind, basis, p):
    return types.SimpleNamespace(constProj_rest_shape="first", constProj_numFrames=0, constProj_p_size=p,
                                 constProj_massWeight=False, constProj_standarize=True, constProj_orthogonal=False,
                                 constProj_basis_type=basis, deim_desired_num_components=K,
                                 constProj_store_sing_val=False, constProj_output_directory=str(tmp), name="t", constProj_name="v",
                                 constProj_bases_interpolation_type=kind, constProj_snapshots_type="tris_strain")


def _build(frames, K, tmp, kind="deim", basis="pod_vectorized", p=1, test_frames=None, engine=None, comm=None, comps=None):
    from animsnapbases_amd import constraintsComponents, nonlinearSnapshots
    param = _cparam(K, tmp, kind, basis, p)
    with contextlib.redirect_stdout(io.StringIO()):
        ns = nonlinearSnapshots(param, frames=frames, test_frames=test_frames, engine=engine, comm=comm)
        ns.config()
        ns.snapshots_prepare()
        cc = constraintsComponents(param, ns)
        cc.config()
        if comps is None:
            cc.compute_components_store_singvalues()
        else:
            cc.numComp = K
            cc.comps = comps
    return ns, cc


def _deim(cc):
    with contextlib.redirect_stdout(io.StringIO()):
        cc.deim()


def _synth(ep, F, K, seed, test=0):
    rng = np.random.default_rng(seed)
    modes = rng.normal(size=(K + 20, ep, 3))
    coef = rng.normal(size=(F + test, K + 20)) * (0.93 ** np.arange(K + 20))[None]
    frames = 0.2 + np.tensordot(coef, modes, (1, 0)) + 1e-7 * rng.normal(size=(F + test, ep, 3))
    return frames[:F], (frames[F:] if test else None)


def _host_metrics(cc, r, case):
    from animsnapbases_amd import constraintsComponents as CC
    ns = cc.nonlinearSnapshots
    f = ns.snapTensor if case == "train" else ns.test_snapTensor
    rec = cc.geom_constructed(r, case)
    rel = CC.relative_error_per_component(f, rec)
    return [CC.frobenius_error(f, rec), CC.max_pointwise_error(f, rec), rel[0], rel[1], rel[2]]


def _kappa(cc, r):
    """max over the coordinates of cond(A^T A), A = V[Pt_r, :r]: both the device and the host solve carry ~ kappa eps."""
    Pt = cc.geom_alpha[:cc.geom_alpha_ranges[r - 1]]
    V = cc.comps
    return max(np.linalg.cond(V[:r, Pt, l].T @ V[:r, Pt, l]) for l in range(3))


def _check(got, ref, tol, slack=0.0):
    """got / ref: [fro, max, rx, ry, rz] of one r.  |got - ref| <= tol |ref| + slack (slack: in units of the normalised metric's
    own scale -- the conditioning floor of the two LU solves)."""
    for a, b in zip(got, ref):
        assert abs(a - b) <= tol * abs(b) + slack, (got, ref)


def test_reference_parity_golden(tmp_path):
    from animsnapbases_amd import constraintsComponents as CC
    g = load_golden("pod_deim_small")
    rec = load_golden("pod_deim_recon")
    K = int(g["K"])
    ns, cc = _build(g["frames"], K, tmp_path)
    ns.test_snapTensor = rec["test_snapTensor"]
    _deim(cc)
    assert cc.geom_Pt.tolist() == rec["Pt"].tolist()
    for case, f in (("train", g["snapTensor"]), ("test", rec["test_snapTensor"])):
        got = cc.interpolation_errors([3, K], case)
        for i, r in enumerate((3, K)):
            fr = rec["%s_r%d" % (case, r)]
            rel = CC.relative_error_per_component(f, fr)
            ref = [CC.frobenius_error(f, fr), CC.max_pointwise_error(f, fr), rel[0], rel[1], rel[2]]
            _check([got[j][i] for j in range(5)], ref, 1e-8)


@pytest.mark.parametrize("ep,F,K", [(1000, 70, 40), (5003, 301, 130), (777, 9, 5)])
@pytest.mark.parametrize("post", [False, True])
def test_every_r_equals_geom_constructed(ep, F, K, post, tmp_path):
    frames, test = _synth(ep, F, K, ep + F, test=7)
    ns, cc = _build(frames, K, tmp_path, test_frames=test)
    if post:
        with contextlib.redirect_stdout(io.StringIO()):
            cc.post_process_components()
    _deim(cc)
    for case in ("train", "test"):
        got = cc.interpolation_errors(range(1, K + 1), case)
        for r in range(1, K + 1):
            ref = _host_metrics(cc, r, case)
            # 1e-10 relative; where cond(A^T A) is large, both results carry its rounding: allow 1e-15 kappa of the
            # metric's scale (fro: |f|, max: max|f| / max f, rel: 1)
            f = ns.snapTensor if case == "train" else ns.test_snapTensor
            k = _kappa(cc, r) * 1e-15
            scales = [np.linalg.norm(f), np.abs(f).max() / abs(f.max()), 1.0, 1.0, 1.0]
            for j in range(5):
                assert abs(got[j][r - 1] - ref[j]) <= 1e-10 * abs(ref[j]) + k * scales[j], (case, r, j, got[j][r - 1], ref[j])


def test_block_form_singular_raises(tmp_path):
    g = load_golden("block_deim_p3")
    K, p = int(g["K"]), int(g["p"])
    ns, cc = _build(g["frames"], K, tmp_path, "deim_block_form", "pca_blocks", p)
    with contextlib.redirect_stdout(io.StringIO()):
        cc.deim_blocksForm()
    for r in range(1, K + 1):
        with pytest.raises(ValueError, match="r = %d" % r):
            cc.interpolation_errors([r])


def test_config5_shape(tmp_path):
    ep, F, K = 50000, 4000, 256
    rng = np.random.default_rng(5)
    modes = rng.normal(size=(K + 20, ep * 3))
    coef = rng.normal(size=(F, K + 20)) * (0.97 ** np.arange(K + 20))[None]
    frames = (coef @ modes).reshape(F, ep, 3)
    frames += 1e-6 * rng.standard_normal(size=frames.shape, dtype=np.float32)
    del modes
    ns, cc = _build(frames, K, tmp_path)
    del frames
    with contextlib.redirect_stdout(io.StringIO()):
        cc.post_process_components()
    _deim(cc)
    full = cc.interpolation_errors(range(1, K + 1))
    assert all(np.isfinite(v).all() for v in full)
    spots = [1, 17, 128, 256]
    single = [cc.interpolation_errors([r]) for r in spots]
    for r, one in zip(spots, single):
        assert [v[0] for v in one] == [v[r - 1] for v in full]
    for r in spots:
        ref = _host_metrics(cc, r, "train")
        f = ns.snapTensor
        k = _kappa(cc, r) * 1e-15
        scales = [np.linalg.norm(f), np.abs(f).max() / abs(f.max()), 1.0, 1.0, 1.0]
        for j in range(5):
            assert abs(full[j][r - 1] - ref[j]) <= 1e-10 * abs(ref[j]) + k * scales[j], (r, j, full[j][r - 1], ref[j])


@pytest.mark.parametrize("world", [2, 3])
def test_several_ranks(world, tmp_path):
    from animsnapbases_amd import HipEngine
    from thread_comm import run_ranks
    ep, F, K = 1201, 50, 20
    frames, test = _synth(ep, F, K, world, test=11)
    ns, cc = _build(frames, K, tmp_path, test_frames=test)
    _deim(cc)
    V, alpha, ranges = cc.comps.copy(), cc.geom_alpha.copy(), cc.geom_alpha_ranges.copy()
    rs = list(range(1, K + 1))
    one = [cc.interpolation_errors(rs, "train"), cc.interpolation_errors(rs, "test")]

    def run(rank, comm):
        ns_, cc_ = _build(frames, K, tmp_path, test_frames=test, engine=HipEngine(0, stream=0), comm=comm, comps=V)
        cc_.geom_alpha, cc_.geom_Pt, cc_.geom_alpha_ranges = alpha, alpha, ranges
        return [cc_.interpolation_errors(rs, "train"), cc_.interpolation_errors(rs, "test")]

    outs = run_ranks(world, run)
    for out in outs:
        assert out == outs[0]
        for lists, ref in zip(out, one):
            for a, b in zip(lists, ref):
                a, b = np.asarray(a), np.asarray(b)
                assert np.all(np.abs(a - b) <= 1e-12 * np.abs(b)), (a, b)


def test_deterministic_and_no_big_transfers(tmp_path, monkeypatch):
    from animsnapbases_amd import HipEngine, constraints
    frames, test = _synth(3001, 90, 24, 7, test=5)
    ns, cc = _build(frames, 24, tmp_path, test_frames=test)
    _deim(cc)
    ref = [cc.interpolation_errors(range(1, 25), c) for c in ("train", "test")]

    def boom(*a, **k):
        raise AssertionError("a full-size transfer")
    monkeypatch.setattr(HipEngine, "download_snapshots", boom)
    monkeypatch.setattr(HipEngine, "components_expand", boom)
    ns._snapTensor = None
    for _ in range(2):
        assert [cc.interpolation_errors(range(1, 25), c) for c in ("train", "test")] == ref
    monkeypatch.setattr(constraints, "INTERP_SWEEP_POINTS", 5)          # several reads of the tensor: the same numbers
    assert [cc.interpolation_errors(range(1, 25), c) for c in ("train", "test")] == ref


@pytest.mark.parametrize("steps", [1, 5])
def test_csv_writer(steps, tmp_path):
    frames, test = _synth(900, 40, 12, 3, test=6)
    ns, cc = _build(frames, 12, tmp_path, test_frames=test)
    _deim(cc)
    cc.store_convergence_tests(steps)
    base = os.path.join(str(tmp_path), "t_v_deim_pod_vectorized")
    rs = list(range(1, 13, steps))
    header = ['numPoints', 'fro_error', 'max_err', 'relative_errors_x', 'relative_errors_y', 'relative_errors_z', 'relative3d']
    for case in ("train", "test"):
        rows = list(csv.reader(open(base + "_%s_convergence_tests.csv" % case)))
        assert rows[0] == header and len(rows) == len(rs) + 1
        fro, mx, rx, ry, rz = cc.interpolation_errors(rs, case)
        for i, row in enumerate(rows[1:]):
            assert int(row[0]) == rs[i]
            vals = [float(v) for v in row[1:]]
            assert vals[:5] == [fro[i], mx[i], rx[i], ry[i], rz[i]]
            assert vals[5] == np.sum([rx[i], ry[i], rz[i]]) / 3
    rows = list(csv.reader(open(base + "_num_interpol_elemnets.csv")))
    assert rows[0] == ['numPoints', 'num_elements']
    assert [[int(a), int(b)] for a, b in rows[1:]] == [[r, int(cc.geom_alpha_ranges[r - 1])] for r in range(1, 13)]


def test_refusals(tmp_path):
    frames, test = _synth(500, 30, 8, 1, test=4)
    ns, cc = _build(frames, 8, tmp_path, test_frames=test)
    with pytest.raises(ValueError):
        cc.interpolation_errors([1])                                  # no interpolation points yet
    _deim(cc)
    for bad in ([0], [9], [1, 9]):
        with pytest.raises(ValueError):
            cc.interpolation_errors(bad)
    with pytest.raises(ValueError):
        cc.interpolation_errors([1], "validation")
    cc.geom_alpha_ranges = cc.geom_alpha_ranges.copy()
    cc.geom_alpha_ranges[2] = 2                                       # fewer rows than basis vectors at r = 3
    with pytest.raises(ValueError, match="r = 3"):
        cc.interpolation_errors([1, 2, 3])
    ns.test_snapTensor = None
    with pytest.raises(ValueError):
        cc.interpolation_errors([1], "test")
