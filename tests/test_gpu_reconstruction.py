"""GPU (-m gpu): reconstruction-error sweeps (posComponents.test_convergence / reconstruction_errors, csrc/asb_recon.hip) and
the least-squares projection of a held-out animation (project_animation), against a NumPy restatement of the reference's
formulas (snapbases/posComponents.py:192-249) and numpy.linalg.lstsq."""
import contextlib
import io
import types

import numpy as np
import pytest

from oracle import asb_oracle as orc

pytestmark = pytest.mark.gpu


def _param(**over):
    d = dict(vertPos_bases_type="PCA", vertPos_numComponents=4, q_support="global", store_vertPos_PCA_sing_val=False,
             vertPos_smooth_min_dist=0.1, vertPos_smooth_max_dist=0.3, q_standarize=True, q_massWeight=False,
             q_orthogonal=False, vertPos_output_directory=".", name="recon")
    d.update(over)
    return types.SimpleNamespace(**d)


def _build(verts, K, tris=None, support="global", mode=None, standarize=True, massWeight=False, rest="first", mass=None,
           test_verts=None, engine=None, comm=None, **over):
    from animsnapbases_amd import posComponents, posSnapshots
    with contextlib.redirect_stdout(io.StringIO()):
        snaps = posSnapshots.from_arrays(verts, tris, rest, standarize=standarize, massWeight=massWeight, mass=mass,
                                         test_verts=test_verts, engine=engine, comm=comm)
        comp = posComponents(_param(vertPos_numComponents=K, q_support=support, q_standarize=standarize,
                                    q_massWeight=massWeight, **over), snaps)
        comp.deflate_mode = mode
        comp.compute_components_store_singvalues()
    return snaps, comp


# ---- the model: posComponents.py:192-249 restated (reconstruction = tensordot(weigs[:, :k], comps[:k]))
def model_sweep(T, W, C, ks):
    fro, mx, rx, ry, rz = [], [], [], [], []
    rec = np.zeros_like(T)
    k0 = 0
    for k in ks:
        if k > k0:
            rec += np.tensordot(W[:, k0:k], C[k0:k], axes=([1], [0]))
            k0 = k
        E = T - rec
        fro.append(np.linalg.norm(E))
        rel = [np.linalg.norm(E[:, :, i]) / np.linalg.norm(T[:, :, i]) for i in range(3)]
        rx.append(rel[0])
        ry.append(rel[1])
        rz.append(rel[2])
        mx.append(np.max(np.abs(E)) / np.max(T))
    return fro, mx, rx, ry, rz


def check_lists(got, ref, T, fro_rtol=1e-10):
    nT = np.linalg.norm(T)
    nd = [np.linalg.norm(T[:, :, i]) for i in range(3)]
    tmax, amax = np.max(T), np.max(np.abs(T))
    assert [len(x) for x in got] == [len(x) for x in ref]
    g, r = [np.asarray(x, dtype=np.float64) for x in got], [np.asarray(x, dtype=np.float64) for x in ref]
    assert np.all(np.abs(g[0] - r[0]) <= 1e-12 * nT + fro_rtol * np.abs(r[0])), (g[0], r[0])
    for i, d in zip((2, 3, 4), range(3)):      # relative per axis: compare the absolute errors
        assert np.all(np.abs(g[i] - r[i]) * nd[d] <= 1e-12 * nd[d] + fro_rtol * np.abs(r[i]) * nd[d]), (i, g[i], r[i])
    assert np.all(np.abs(g[1] - r[1]) * abs(tmax) <= 1e-12 * amax), (g[1], r[1])


def _sweeps(K):
    return [(0, K, 1), (3, K, 5), (K, K, 1)]


@pytest.mark.parametrize("F,N,K", [(1, 7, 1), (17, 1000, 9), (200, 5000, 32), (2049, 3000, 40)])
@pytest.mark.parametrize("mode", ["residual", "project"])
def test_train_sweep_vs_model(F, N, K, mode):
    rng = np.random.default_rng(F + N)
    verts = rng.uniform(-1, 1, size=(F, N, 3))
    snaps, comp = _build(verts, K, mode=mode, standarize=F > 1)
    T, W, C = snaps.snapTensor, comp.weigs, comp.comps
    for start, end, step in _sweeps(K):
        got = comp.reconstruction_errors(start, end, step)
        check_lists(got, model_sweep(T, W, C, range(start, end + 1, step)), T)
        assert got == comp.reconstruction_errors(start, end, step)           # bit-identical on a second call
    assert comp.test_convergence(0, K, 1) == comp.reconstruction_errors(0, K, 1)


def test_train_sweep_local_support():
    rest, tris = orc.synth_mesh(8, 12, seed=3)
    verts = orc.synth_snapshots(rest, 30, rank=5, seed=3, kind="bumps")
    K = 6
    snaps, comp = _build(verts, K, tris=tris, support="local")
    T = snaps.snapTensor
    for start, end, step in _sweeps(K):
        got = comp.reconstruction_errors(start, end, step)
        check_lists(got, model_sweep(T, comp.weigs, comp.comps, range(start, end + 1, step)), T)
        assert got == comp.reconstruction_errors(start, end, step)


def test_config4_convergence_without_download(tmp_path):
    """Config 4 (100 000 x 2 000, K = 128, global support): the 1..128 sweep reads the tensor in HBM; its Frobenius errors
    are the residual norms of the deflation (R_k = X - W_k C_k)."""
    from animsnapbases_amd import posComponents, posSnapshots
    from conftest import load_golden
    from config_fixtures import c4_frames, make_param
    g = load_golden("c4_uniform_pca_global")
    verts = c4_frames(g)
    param = make_param(g, vertPos_output_directory=str(tmp_path))
    snaps = posSnapshots.from_arrays(verts, None, param.vertPos_rest_shape, standarize=param.q_standarize,
                                     massWeight=param.q_massWeight)
    del verts
    comp = posComponents(param, snaps)
    comp.compute_components_store_singvalues()
    K = comp.numComp
    assert K == 128
    fro, mx, rx, ry, rz = comp.test_convergence(1, K, 1)
    normX = comp.reconstruction_errors(0, 0, 1)[0][0]
    assert snaps._snapTensor is None
    normR = comp.measures_at_largeDeforVerts[:, 2]
    assert np.all(np.abs(np.asarray(fro) - normR) <= 1e-9 * normX)
    assert np.all(np.diff(fro) <= 1e-9 * normX) and np.all(np.isfinite(mx + rx + ry + rz))


def test_per_axis_and_max_at_20000_by_2049():
    rng = np.random.default_rng(11)
    verts = rng.uniform(-1, 1, size=(2049, 20000, 3))
    K = 128
    snaps, comp = _build(verts, K)
    del verts
    got = comp.reconstruction_errors(1, K, 1)
    T = snaps.snapTensor
    ks = [1, 37, 128]
    ref = model_sweep(T, comp.weigs, comp.comps, ks)
    check_lists([[x[k - 1] for k in ks] for x in got], ref, T)


def test_after_post_processing_and_setter():
    rng = np.random.default_rng(2)
    rest, tris = orc.synth_mesh(10, 14, seed=2)
    verts = orc.synth_snapshots(rest, 60, rank=8, seed=2)
    N, K = verts.shape[1], 8
    mass = rng.uniform(0.5, 2.0, size=N)
    snaps, comp = _build(verts, K, tris=tris, massWeight=True, mass=mass, q_orthogonal=True)
    with contextlib.redirect_stdout(io.StringIO()):
        comp.post_process_components()
    T = snaps.snapTensor
    for start, end, step in _sweeps(K):
        got = comp.reconstruction_errors(start, end, step)
        check_lists(got, model_sweep(T, comp.weigs, comp.comps, range(start, end + 1, step)), T)
    C2 = rng.normal(size=comp.comps.shape) * 0.1
    comp.comps = C2
    got = comp.reconstruction_errors(0, K, 1)
    check_lists(got, model_sweep(T, comp.weigs, C2, range(0, K + 1)), T)


# ---- held-out animations against numpy.linalg.lstsq
def _transform(snaps, Y):
    Yp = np.array(Y, dtype=np.float64)
    if snaps.massL is not None:
        Yp = Yp * snaps.massL[None, :, None]
    if snaps._standarize:
        Yp = (Yp - snaps.mean[None]) * snaps.pre_scale_factor
    return Yp


def _lstsq_model(Yp, C, ks):
    Fp = Yp.shape[0]
    Yf = Yp.reshape(Fp, -1)
    fro, mx, rx, ry, rz, Ws = [], [], [], [], [], {}
    for k in ks:
        if k == 0:
            rec = np.zeros_like(Yp)
        else:
            Wk = np.linalg.lstsq(C[:k].reshape(k, -1).T, Yf.T, rcond=None)[0].T
            Ws[k] = Wk
            rec = (Wk @ C[:k].reshape(k, -1)).reshape(Yp.shape)
        E = Yp - rec
        fro.append(np.linalg.norm(E))
        rel = [np.linalg.norm(E[:, :, i]) / np.linalg.norm(Yp[:, :, i]) for i in range(3)]
        rx.append(rel[0])
        ry.append(rel[1])
        rz.append(rel[2])
        mx.append(np.max(np.abs(E)) / np.max(Yp))
    return (fro, mx, rx, ry, rz), Ws


@pytest.mark.parametrize("Ft", [37, 2100])
@pytest.mark.parametrize("std,mw,rest", [(True, True, "first"), (False, False, "first"), (True, False, "average")])
def test_heldout_vs_lstsq(Ft, std, mw, rest):
    rng = np.random.default_rng(Ft)
    F, N, K = 120, 3000, 24
    base = rng.uniform(-1, 1, size=(N, 3))
    modes = rng.normal(size=(12, N, 3))
    verts = base + np.tensordot(rng.normal(size=(F, 12)), modes, axes=1) + 0.05 * rng.normal(size=(F, N, 3))
    Y = base + np.tensordot(rng.normal(size=(Ft, 12)), modes, axes=1) + 0.05 * rng.normal(size=(Ft, N, 3))
    mass = rng.uniform(0.5, 2.0, size=N) if mw else None
    snaps, comp = _build(verts, K, standarize=std, massWeight=mw, rest=rest, mass=mass, test_verts=Y)
    C = comp.comps
    Yp = _transform(snaps, Y)
    for start, end, step in _sweeps(K):
        ks = list(range(start, end + 1, step))
        got = comp.reconstruction_errors(start, end, step, "test")
        ref, _ = _lstsq_model(Yp, C, ks)
        check_lists(got, ref, Yp, fro_rtol=1e-9)
        assert got == comp.reconstruction_errors(start, end, step, "test")
    Wg = comp.project_animation()
    _, Ws = _lstsq_model(Yp, C, [K])
    assert Wg.shape == (Ft, K)
    assert np.abs(Wg - Ws[K]).max() <= 1e-10 * np.abs(Ws[K]).max()
    assert np.array_equal(comp.project_animation(Y), Wg)

    # Y' inside span(C_k): error ~ 0 from k on
    k = 5
    Yin = np.tensordot(rng.normal(size=(Ft, k)), C[:k], axes=1)
    Yraw = Yin / snaps.pre_scale_factor + snaps.mean[None] if std else Yin.copy()
    if mw:
        Yraw = Yraw / snaps.massL[None, :, None]
    Yinp = _transform(snaps, Yraw)
    fro = comp.reconstruction_errors(0, K, 1, Yraw)[0]
    assert max(fro[k:]) <= 1e-10 * np.linalg.norm(Yinp)

    # the training verts as a held-out animation: the same tensor (k = 0) and never worse than the greedy weights
    tr = comp.reconstruction_errors(0, K, 1, "train")
    ho = comp.reconstruction_errors(0, K, 1, verts)
    for a, b in zip(tr, ho):
        assert abs(a[0] - b[0]) <= 1e-14 * abs(a[0])
    nX = tr[0][0]
    assert np.all(np.asarray(ho[0]) <= np.asarray(tr[0]) + 1e-10 * nX)


def test_heldout_duplicated_component():
    rng = np.random.default_rng(9)
    verts = rng.uniform(-1, 1, size=(80, 2000, 3))
    K = 10
    Y = rng.uniform(-1, 1, size=(50, 2000, 3))
    snaps, comp = _build(verts, K, test_verts=Y)
    C = comp.comps.copy()
    comp.comps = np.concatenate([C[:4], C[3:4], C[4:K - 1]])          # c_4 == c_3
    fro, mx, rx, ry, rz = comp.reconstruction_errors(0, K, 1, "test")
    assert np.all(np.isfinite(fro + mx + rx + ry + rz))
    assert abs(fro[4] - fro[5]) <= 1e-12 * fro[0]
    assert abs(mx[4] - mx[5]) <= 1e-12 * abs(mx[0])
    W = comp.project_animation()
    assert np.all(np.isfinite(W)) and np.all(W[:, 4] == 0.0)


@pytest.mark.parametrize("world", [2, 3])
def test_multirank_equals_single_rank(world):
    from animsnapbases_amd import HipEngine
    from thread_comm import run_ranks
    rng = np.random.default_rng(world)
    verts = rng.uniform(-1, 1, size=(64, 3001, 3))
    Y = rng.uniform(-1, 1, size=(45, 3001, 3))
    K = 12
    C_fix = rng.normal(size=(K, 3001, 3))

    def run(engine=None, comm=None):
        snaps, comp = _build(verts, K, mode="residual", test_verts=Y, engine=engine, comm=comm)
        tr = comp.reconstruction_errors(0, K, 1)
        W, Cg = comp.weigs.copy(), comp.comps.copy()
        comp.comps = C_fix
        ho = comp.reconstruction_errors(0, K, 1, "test")
        return tr, ho, W, Cg

    tr1, ho1, _, _ = run()
    outs = run_ranks(world, lambda rank, comm: run(HipEngine(0, stream=0), comm))
    for tr, ho, W, Cg in outs:
        for a, b in zip(tr + ho, tr1 + ho1):
            a, b = np.asarray(a), np.asarray(b)
            assert np.all(np.abs(a - b) <= 1e-12 * np.abs(b)), (a, b)
        assert tr == outs[0][0] and ho == outs[0][1]


def test_errors():
    from animsnapbases_amd import posComponents, posSnapshots
    rng = np.random.default_rng(0)
    verts = rng.uniform(-1, 1, size=(20, 50, 3))
    with contextlib.redirect_stdout(io.StringIO()):
        snaps = posSnapshots.from_arrays(verts, None, "first")
    bare = posComponents(_param(vertPos_numComponents=4), snaps)
    with pytest.raises(ValueError):
        bare.reconstruction_errors(0, 4, 1)
    with pytest.raises(ValueError):
        bare.test_convergence(0, 4, 1)
    _, comp = _build(verts, 4)
    with pytest.raises(ValueError):
        comp.reconstruction_errors(0, 4, 1, "test")                  # no test animation
    with pytest.raises(ValueError):
        comp.project_animation()
    with pytest.raises(ValueError):
        comp.reconstruction_errors(0, 4, 1, verts[:, :49])          # N mismatch
    with pytest.raises(ValueError):
        comp.project_animation(verts[:, :49])
    for bad in [(-1, 4, 1), (0, 5, 1), (0, 4, 0)]:
        with pytest.raises(ValueError):
            comp.reconstruction_errors(*bad)
    assert len(comp.reconstruction_errors(0, 4, 1)[0]) == 5


def test_sweep_point_beyond_the_weight_columns_is_refused():
    """a residual run of K = 4 leaves four weight columns; an uploaded basis of six rows does not add any"""
    from animsnapbases_amd import HipEngine
    rng = np.random.default_rng(5)
    X = rng.uniform(-1, 1, size=(20, 50, 3))
    e = HipEngine(0)
    try:
        e.upload(X, 0, 50)
        e.deflate_begin(4, False)
        e.run_global(0, 4)
        e.components_upload(rng.normal(size=(6, 50, 3)))
        with pytest.raises(RuntimeError, match="asb_recon_sweep: k = 5 but 6 components and 4 weight columns"):
            e.recon_sweep(0, [0, 5])
        assert e.recon_sweep(0, [0, 4])[0].shape == (2, 3)
    finally:
        e.close()
