"""GPU (-m gpu): on-mesh accuracy maps (posComponents.on_mesh_accuracy / store_on_mesh_measures, csrc/asb_onmesh.hip) against the
NumPy restatement of compute_accuracy (tests/onmesh_model.py; generate_figures/onMesh_accuracyMeasures.py:61-151).  The
restatement is applied to the world-space input frames and to the reconstruction formed on the host from the downloaded
``weigs`` and ``comps`` (held-out: numpy.linalg.lstsq), mapped back to world space.

Tolerances.  Error maps and mesh_err are sums of squares of the differences asb_recon_sweep forms: 1e-10 relative (held-out
1e-9) beside 1e-12 of the |x|^2 scale, which for frame_err = |x - x_r|^2 / |x|^2 / denom is 1e-12 / denom per entry.  Angles:
a rounding d <= 16 eps of the cosine moves arccos by at most sqrt(2 d) = 8.4e-8 rad = 4.8e-6 degrees: 1e-5 degrees per entry,
F_sel x 1e-5 for sums over the frames.  tests/test_onmesh_cpu.py checks what this assumes of the inputs."""
import contextlib
import csv
import io
import types

import numpy as np
import pytest

import onmesh_cases as oc
import onmesh_model as om

pytestmark = pytest.mark.gpu

ANGLE_TOL = 1e-5


def _param(**over):
    d = dict(vertPos_bases_type="PCA", vertPos_numComponents=4, q_support="global", store_vertPos_PCA_sing_val=False,
             vertPos_smooth_min_dist=0.1, vertPos_smooth_max_dist=0.3, q_standarize=True, q_massWeight=False,
             q_orthogonal=False, vertPos_output_directory=".", name="onmesh")
    d.update(over)
    return types.SimpleNamespace(**d)


def _build(verts, K, tris=None, standarize=True, massWeight=False, rest="first", mass=None, test_verts=None, engine=None,
           comm=None, **over):
    from animsnapbases_amd import posComponents, posSnapshots
    with contextlib.redirect_stdout(io.StringIO()):
        snaps = posSnapshots.from_arrays(verts, tris, rest, standarize=standarize, massWeight=massWeight, mass=mass,
                                         test_verts=test_verts, engine=engine, comm=comm)
        comp = posComponents(_param(vertPos_numComponents=K, q_standarize=standarize, q_massWeight=massWeight, **over), snaps)
        comp.compute_components_store_singvalues()
    return snaps, comp


def _to_world(snaps, Tp):
    X = np.array(Tp, dtype=np.float64)
    if snaps._standarize:
        X = X / snaps.pre_scale_factor + snaps.mean[None]
    if snaps.massL is not None:
        X = X / snaps.massL[None, :, None]
    return X


def _transform(snaps, Y):
    Yp = np.array(Y, dtype=np.float64)
    if snaps.massL is not None:
        Yp = Yp * snaps.massL[None, :, None]
    if snaps._standarize:
        Yp = (Yp - snaps.mean[None]) * snaps.pre_scale_factor
    return Yp


def _reduced_train(snaps, comp, r):
    return _to_world(snaps, np.tensordot(comp.weigs[:, :r], comp.comps[:r], axes=([1], [0])))


def _reduced_heldout(snaps, comp, Y, r):
    Yp = _transform(snaps, Y)
    if r == 0:
        return _to_world(snaps, np.zeros_like(Yp))
    Cr = comp.comps[:r].reshape(r, -1)
    W = np.linalg.lstsq(Cr.T, Yp.reshape(Yp.shape[0], -1).T, rcond=None)[0].T
    return _to_world(snaps, (W @ Cr).reshape(Yp.shape))


def _close(got, ref, rtol, atol, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(np.where(fin, 0.0, got), np.where(fin, 0.0, ref), equal_nan=True), what       # inf / NaN where the model has them
    err = np.abs(got[fin] - ref[fin])
    bound = atol + rtol * np.abs(ref[fin])
    worst = float((err / bound).max()) if err.size else 0.0
    print("%-12s max |got - ref| / bound = %.3g" % (what, worst))
    assert worst <= 1.0, (what, worst)


def check(got, ref, fs, fe, fj, N, normals, rtol=1e-10, per_frame=False):
    n_sel = len(range(fs, fe, fj))
    a1 = 1e-12 / om.denominator(fs, fe, N)
    _close(got["accum_norm"], ref["accum_norm"], rtol, n_sel * a1, "accum_norm")
    _close(got["mesh_err"], ref["mesh_err"], rtol, a1, "mesh_err")
    row = om.stats_row(ref)
    st = got["stats"]
    assert st.shape == (14,)
    _close(st[[0, 2]], row[[0, 2]], rtol, a1, "fe min/max")
    _close(st[[1]], row[[1]], rtol, a1, "fe mean")
    _close(st[[3]], row[[3]], rtol, n_sel * N * a1, "fe sum")
    _close(st[8:11], row[8:11], rtol, n_sel * a1, "accum_norm st")
    if per_frame:
        _close(got["frame_err"], ref["frame_err"], rtol, a1, "frame_err")
    if normals:
        _close(got["accum_angle"], ref["accum_angle"], 0.0, n_sel * ANGLE_TOL, "accum_angle")
        _close(st[[4, 5, 6]], row[[4, 5, 6]], 0.0, ANGLE_TOL, "angle st")
        _close(st[[7]], row[[7]], 0.0, n_sel * N * ANGLE_TOL, "angle sum")
        _close(st[11:14], row[11:14], 0.0, n_sel * ANGLE_TOL, "accum_angle st")
        if per_frame:
            _close(got["angle"], ref["angle"], 0.0, ANGLE_TOL, "angle")
    else:
        assert "accum_angle" not in got and "angle" not in got
        assert np.all(np.isnan(st[4:8])) and np.all(np.isnan(st[11:14]))


@pytest.mark.parametrize("name", sorted(oc.CASES))
def test_train_vs_model(name):
    spec, F, K, std, mw, rest, (fs, fe, fj), rs, nm = oc.CASES[name]
    verts, tris, mass = oc.make_case(name)
    N = verts.shape[1]
    snaps, comp = _build(verts, K, tris=tris, standarize=std, massWeight=mw, rest=rest, mass=mass)
    small = F * N <= 1 << 20
    for r, normals in zip(rs, nm):
        ref = om.compute_accuracy(verts, _reduced_train(snaps, comp, r), tris, fs, fe, fj, normals)
        got = comp.on_mesh_accuracy(r, fs, fe, fj, normals=normals, per_frame=small)
        assert sorted(got) == sorted(["accum_norm", "mesh_err", "stats"] + (["accum_angle"] if normals else [])
                                     + ((["frame_err"] + (["angle"] if normals else [])) if small else []))
        check(got, ref, fs, fe, fj, N, normals, per_frame=small)
    if small and F > 1:          # the whole animation with the defaults (frame_end = None -> F)
        r = rs[-1]
        ref = om.compute_accuracy(verts, _reduced_train(snaps, comp, r), tris, 0, F, 1)
        check(comp.on_mesh_accuracy(r), ref, 0, F, 1, N, True)


@pytest.mark.parametrize("how", ["test", "array"])
def test_heldout_vs_model(how):
    name = "grid1000_F17"
    spec, F, K, std, mw, rest, _, rs, nm = oc.CASES[name]
    verts, tris, mass = oc.make_case(name)
    Y = oc.make_case(name, n_frames=37, seed_shift=1)[0]
    N = verts.shape[1]
    snaps, comp = _build(verts, K, tris=tris, standarize=std, massWeight=mw, rest=rest, mass=mass,
                         test_verts=Y if how == "test" else None)
    for r in rs:
        ref = om.compute_accuracy(Y, _reduced_heldout(snaps, comp, Y, r), tris, 3, 37, 3)
        got = comp.on_mesh_accuracy(r, 3, 37, 3, animation="test" if how == "test" else Y, per_frame=True)
        check(got, ref, 3, 37, 3, N, True, rtol=1e-9, per_frame=True)
    with pytest.raises(ValueError):
        comp.on_mesh_accuracy(1, 0, 38, 1, animation="test" if how == "test" else Y)          # frame_end > F'


def test_isolated_vertex_and_zero_position():
    """A vertex in no triangle: NaN angles.  A position exactly at the origin: inf (or NaN) errors -- without mass weighting
    and standardising, where the tensor holds the input bit for bit (the way back through a mean and a scale is not exact)."""
    rest, tris = om.grid_mesh(9, 11)
    edge = 0.05
    rest = np.concatenate([rest, [[0.3, 0.3, 2.5]]])                     # vertex N - 1: in no triangle
    verts = om.animate(rest, 20, 14, 5, edge)
    verts[7, 40] = 0.0
    N, K, r = rest.shape[0], 6, 3
    snaps, comp = _build(verts, K, tris=tris, standarize=False, massWeight=False)
    ref = om.compute_accuracy(verts, _reduced_train(snaps, comp, r), tris, 0, 20, 1)
    assert np.all(np.isnan(ref["angle"][:, N - 1])) and np.isinf(ref["frame_err"][7, 40]) and np.isinf(ref["accum_norm"][40])
    got = comp.on_mesh_accuracy(r, per_frame=True)
    check(got, ref, 0, 20, 1, N, True, per_frame=True)
    assert np.all(np.isnan(got["angle"][:, N - 1])) and np.isnan(got["accum_angle"][N - 1])
    assert np.isinf(got["frame_err"][7, 40]) and np.isinf(got["stats"][2]) and np.all(np.isnan(got["stats"][4:8]))


def test_per_frame_stats_csv_and_repeats(tmp_path):
    name = "sphere642_F256"
    spec, F, K, std, mw, rest, _, rs, nm = oc.CASES[name]
    verts, tris, mass = oc.make_case(name)
    N = verts.shape[1]
    snaps, comp = _build(verts, K, tris=tris, standarize=std, massWeight=mw, rest=rest, mass=mass)
    fs, fe, fj = 10, 250, 3
    n_sel = len(range(fs, fe, fj))
    a1 = 1e-12 / om.denominator(fs, fe, N)
    for normals in (True, False):
        a = comp.on_mesh_accuracy(16, fs, fe, fj, normals=normals, per_frame=True)
        b = comp.on_mesh_accuracy(16, fs, fe, fj, normals=normals, per_frame=True)
        assert sorted(a) == sorted(b)
        for key in a:                                                       # bit-identical on a second call
            assert np.array_equal(a[key], b[key], equal_nan=True), key
        c = comp.on_mesh_accuracy(16, fs, fe, fj, normals=normals)
        for key in c:                                                       # and the maps change nothing else
            assert np.array_equal(a[key], c[key], equal_nan=True), key
        assert a["frame_err"].shape == (n_sel, N)
        s = a["frame_err"].sum(axis=0)
        assert np.all(np.abs(s - a["accum_norm"]) <= 1e-12 * np.abs(s))
        st = a["stats"]
        row = om.stats_row(a)                                               # the statistics of the maps themselves
        _close(st[[0, 1, 2]], row[[0, 1, 2]], 1e-10, a1, "fe st")
        _close(st[[3]], row[[3]], 1e-10, n_sel * N * a1, "fe sum")
        _close(st[8:11], row[8:11], 1e-10, n_sel * a1, "an st")
        if normals:
            s = a["angle"].sum(axis=0)
            assert np.all(np.abs(s - a["accum_angle"]) <= 1e-12 * np.abs(s))
            _close(st[[4, 5, 6]], row[[4, 5, 6]], 0.0, ANGLE_TOL, "angle st")
            _close(st[[7]], row[[7]], 0.0, n_sel * N * ANGLE_TOL, "angle sum")
            _close(st[11:14], row[11:14], 0.0, n_sel * ANGLE_TOL, "aa st")
    rows = comp.store_on_mesh_measures([0, 8, 32], str(tmp_path), frame_start=fs, frame_end=fe, frame_jump=fj)
    with open(tmp_path / "_on_mesh_measures_test_on_training_set.csv", encoding="UTF8") as fh:
        lines = list(csv.reader(fh))
    assert lines[0] == om.HEADER and len(lines) == 4
    for line, r, row in zip(lines[1:], [0, 8, 32], rows):
        st = comp.on_mesh_accuracy(r, fs, fe, fj)["stats"]
        assert int(line[0]) == r and row[0] == r
        assert np.array_equal(np.array([float(x) for x in line[1:]]), st, equal_nan=True)
    comp.store_on_mesh_measures([8], str(tmp_path), case="_b", normals=False)
    assert (tmp_path / "_on_mesh_measures_b.csv").exists()


def test_without_triangles():
    rng = np.random.default_rng(4)
    verts = rng.uniform(1, 2, size=(40, 500, 3))
    snaps, comp = _build(verts, 8, tris=None)
    ref = om.compute_accuracy(verts, _reduced_train(snaps, comp, 4), None, 0, 40, 1, normals=False)
    check(comp.on_mesh_accuracy(4, normals=False, per_frame=True), ref, 0, 40, 1, 500, False, per_frame=True)
    with pytest.raises(ValueError):
        comp.on_mesh_accuracy(4)                                            # normals=True and no triangles


@pytest.mark.parametrize("world", [2, 3])
def test_multirank_equals_single_rank(world):
    from animsnapbases_amd import HipEngine
    from thread_comm import run_ranks
    name = "grid1000_F17"
    verts, tris, mass = oc.make_case(name)
    Y = oc.make_case(name, n_frames=21, seed_shift=2)[0]
    K = 8

    def run(engine=None, comm=None):
        snaps, comp = _build(verts, K, tris=tris, massWeight=True, mass=mass, test_verts=Y, engine=engine, comm=comm)
        outs = [comp.on_mesh_accuracy(4, 2, 17, 3, normals=False, per_frame=True),
                comp.on_mesh_accuracy(8, 1, 20, 2, animation="test", normals=False)]
        if comm is not None:
            with pytest.raises(NotImplementedError):
                comp.on_mesh_accuracy(4, 2, 17, 3)
        return outs

    one = run()
    for outs in run_ranks(world, lambda rank, comm: run(HipEngine(0, stream=0), comm)):
        for got, ref in zip(outs, one):
            assert sorted(got) == sorted(ref)
            for key in ("accum_norm", "mesh_err", "frame_err"):
                if key in ref:
                    assert np.all(np.abs(got[key] - ref[key]) <= 1e-12 * np.abs(ref[key])), key
            fin = np.isfinite(ref["stats"])
            assert np.array_equal(fin, np.isfinite(got["stats"]))
            assert np.all(np.abs(got["stats"][fin] - ref["stats"][fin]) <= 1e-12 * np.abs(ref["stats"][fin]))


def test_refusals():
    verts, tris, mass = oc.make_case("grid1000_F17")
    K, F = 8, 17
    snaps, comp = _build(verts, K, tris=tris)
    for bad in [dict(r=-1), dict(r=K + 1), dict(r=2, frame_start=5, frame_end=5), dict(r=2, frame_start=9, frame_end=4),
                dict(r=2, frame_jump=0), dict(r=2, frame_end=F + 1), dict(r=2, frame_start=-1), dict(r=2, animation="other"),
                dict(r=2, animation="test")]:
        with pytest.raises(ValueError):
            comp.on_mesh_accuracy(**bad)
    before = comp.on_mesh_accuracy(2)
    with contextlib.redirect_stdout(io.StringIO()):
        comp.post_process_components()
    with pytest.raises(ValueError):
        comp.on_mesh_accuracy(2)                                            # the basis left the tensor's space
    with pytest.raises(ValueError):
        comp.store_on_mesh_measures([2], ".")
    with contextlib.redirect_stdout(io.StringIO()):
        comp.compute_components_store_singvalues()
    after = comp.on_mesh_accuracy(2)
    for key in before:
        assert np.allclose(before[key], after[key], rtol=1e-9, atol=0.0, equal_nan=True), key
    with contextlib.redirect_stdout(io.StringIO()):
        comp.post_process_components()
    comp.comps = np.array(comp.comps)                                       # the setter clears the refusal too
    assert comp.on_mesh_accuracy(2)["accum_norm"].shape == (verts.shape[1],)


def test_r_beyond_the_weight_columns_is_refused():
    """a residual run of K = 4 leaves four weight columns; an uploaded basis of six rows does not add any"""
    from animsnapbases_amd import HipEngine
    rng = np.random.default_rng(6)
    X = rng.uniform(-1, 1, size=(20, 50, 3))
    e = HipEngine(0)
    try:
        e.upload(X, 0, 50)
        e.deflate_begin(4, False)
        e.run_global(0, 4)
        e.components_upload(rng.normal(size=(6, 50, 3)))
        with pytest.raises(RuntimeError, match="asb_onmesh_run: r = 5 but 6 components and 4 weight columns"):
            e.onmesh_run(0, 5, 0, 20, 1, False, None, False, 1.0, 1.0)
        assert e.onmesh_run(0, 4, 0, 20, 1, False, None, False, 1.0, 1.0)["accum_norm"].shape == (50,)
    finally:
        e.close()
