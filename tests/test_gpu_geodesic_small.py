"""GPU (-m gpu): the device geodesics of csrc/asb_geodesic.hip on the small meshes of tests/geodesic_cases.py -- the padding,
tile and threshold edges that the workload's own meshes never reach -- through the existing entry points and four read-only
hooks (asb_test_slab_gemm64, asb_test_geodesic_field1, asb_test_support_weights, asb_test_geodesic_cached), against
tests/geodesic_model.py run in numpy.longdouble on the operators the device holds.

Groups: a. slab_gemm64 alone; b. dense mode, 64-wide batch path; c. dense mode, single-source path and k_support_weights;
d. slab mode (block-tridiagonal LDL^T) with small, ragged slabs; e. sparse mode on either side of n = 512; f. the field cache;
g. a second, third, ... set-up on one engine; h. host-side refusals (none launches a kernel).

Tolerances.  For every compared quantity the float64 model's deviation from the longdouble model on the same inputs is measured
(relative Frobenius norm; largest entry of the difference over the largest entry); the device may deviate from the longdouble
model by the largest of MARGIN = 100 times that, FLOOR = 50 eps and, for the iterative solves of the sparse mode only,
kappa * 1e-13 (kappa: the 2-norm condition number of -L on the mean-free space; below 512 vertices, where the heat step is a PCG
solve too, the larger of that and cond(A - tL)).  Margin and floor are those of tests/test_gpu_splocs_phases.py, for the same
reason: another order of summation, Gauss-Jordan inverses where the model factorises -- and here the three forms of the singular
Poisson step (gauge term, grounded vertex, PCG in the range), which differ by cond(-L) eps on a float64 L whose rows sum to zero
only up to rounding.  No bound may exceed the acceptance levels of tests/test_gpu_geodesic_pcg.py, 1e-9 (dense, slab) and 1e-8
(sparse): check() asserts that, tests/test_geodesic_model_cpu.py establishes it for every case on the CPU.  A batch of 1 against a
batch of 64, and a re-used engine against a fresh one, must agree within FLOOR.  Exact zeros, the clamps of the support weights,
untouched columns and cached fields are compared bit for bit.

Largest deviation of the device from the longdouble model observed on an MI355X, per group (relative Frobenius norm / largest
entry), next to the smallest bound any case of the group had:

    group       quantity      observed fro   observed max   smallest bound
    a gemm64    out           2.5e-16        4.0e-16        1.3e-14
    b dense     phi           5.7e-14        4.9e-14        3.0e-14
    c single    phi           3.6e-14        4.3e-14        4.4e-14
    c single    s (abs.)      2.5e-16        2.5e-16        8.9e-16
    d slab      phi           5.8e-14        7.8e-14        3.0e-14
    e sparse    phi           1.2e-12        2.4e-12        3.0e-11
    e sparse    solve_many    3.3e-15        8.1e-15        4.2e-11
    g re-setup  field1        7.1e-15        6.5e-15        6.2e-14
    g re-setup  phi           1.0e-14        1.0e-14        4.4e-14

(The largest deviations belong to the cases with the largest bounds -- n600, stride: bound 2e-12 .. 6e-12 -- not to the cases of
the smallest.)  A batch of 1 and a batch of 64 were bit-identical in the dense and the slab mode and differed by 2e-15 in the
sparse mode; a re-used engine was bit-identical to a fresh one in every step.  Heat sweeps: 2176 (n512), 2624 (n600), 4928
(stride) against predictions of 2222, 2663 and 4246; Poisson iterations 100 .. 175.  The table was taken before the first
direction of k_cg_direction stopped reading the uninitialised p: until then the two Jacobi-only PCG cases of group e (n127,
n511) returned NaN whenever p held NaN from an earlier batch, so "e sparse" has their figures from single first solves on a
fresh engine only (deviation 5.8e-14 and 2.4e-12, bounds 3.6e-11 and 3.0e-11); they have not been re-measured since.
"""
import functools

import numpy as np
import pytest

import geodesic_cases as gc
import geodesic_model as gm

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
MARGIN, FLOOR = 100.0, 50 * EPS
CEIL_DIRECT, CEIL_SPARSE = 1e-9, 1e-8
TOL = 1e-13
LD = np.longdouble
BATCHES_DENSE = (1, 15, 16, 17, 33, 48, 49, 64)
BATCHES = (1, 17, 64)

_SEEN = {}              # (group, quantity) -> [largest fro, largest max, smallest bound]
_FRESH = {}             # (case, backend) -> fields of a fresh engine (group g)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _SEEN:
        print("\n    group       quantity      observed fro   observed max   smallest bound")
        for (group, name), (fro, mx, bound) in sorted(_SEEN.items()):
            print("    %-11s %-13s %-14.1e %-14.1e %.1e" % (group, name, fro, mx, bound))


def check(group, name, got, lo, hi, where, extra=0.0, ceil=CEIL_DIRECT):
    """got (device) against hi (longdouble model) within the largest of MARGIN times the deviation of lo (float64 model) from hi,
    FLOOR and `extra` (kappa * tol of an iterative solve)"""
    got = np.asarray(got)
    assert np.isfinite(got).all(), (group, name, where, "not finite")
    ref_fro, ref_max = gm.deviation(lo, hi)
    b_fro, b_max = max(FLOOR, MARGIN * ref_fro, extra), max(FLOOR, MARGIN * ref_max, extra)
    assert b_fro <= ceil and b_max <= ceil, (group, name, where, "the reference alone is above the ceiling", ref_fro, ref_max, extra)
    fro, mx = gm.deviation(got, hi)
    print("%s %s %s: device %.2e / %.2e, float64 model %.2e / %.2e, bound %.2e / %.2e" % (group, name, where, fro, mx, ref_fro, ref_max,
                                                                                           b_fro, b_max))
    seen = _SEEN.setdefault((group, name), [0.0, 0.0, np.inf])
    seen[0], seen[1], seen[2] = max(seen[0], fro), max(seen[1], mx), min(seen[2], b_fro, b_max)
    assert fro <= b_fro and mx <= b_max, (group, name, where, fro, b_fro, mx, b_max)


def same(group, a, b, where):
    """two device results that may differ by FLOOR at the most; prints whether they are bit-identical"""
    fro, mx = gm.deviation(a, b)
    print("%s %s: %s (%.2e / %.2e)" % (group, where, "bit-identical" if np.array_equal(a, b) else "NOT bit-identical", fro, mx))
    assert fro <= FLOOR and mx <= FLOOR, (group, where, fro, mx)


def _engine():
    from animsnapbases_amd import HipEngine
    return HipEngine(0)


def _setup(eng, name, backend, monkeypatch=None, target=None):
    """a prepared GeodesicDistanceComputation of the case on `eng`; slab mode with bfs_slabs' target replaced when given"""
    import animsnapbases_amd.geodesic as geomod
    if target is not None:
        monkeypatch.setattr(geomod, "bfs_slabs", functools.partial(geomod.bfs_slabs, target=target))
    V, T = gc.mesh(name)
    return geomod.GeodesicDistanceComputation(V, T, engine=eng, backend=backend).prepare()


def _check_fields(group, name, phi, src, where, **kw):
    ref = gm.reference(name)
    for q, s in enumerate(src):
        assert phi[q].min() == 0.0, (group, name, where, "min shift")
        check(group, "phi", phi[q], gm.rows(ref, "lo", [s])[0], gm.rows(ref, "hi", [s])[0], "%s %s source %d" % (name, where, s), **kw)


def _batches(group, eng, name, batches, **kw):
    """every batch size against the model; the duplicate pair bit for bit; a batch of 1 against a batch of 64"""
    n = gc.mesh(name)[0].shape[0]
    out = {}
    for k in batches:
        src = gc.sources(n, k)
        phi, its = eng.geodesic_solve(src, TOL)
        assert phi.shape == (k, n)
        _check_fields(group, name, phi, src, "nsrc=%d" % k, **kw)
        if k > 1:
            assert src[0] == src[-1] and np.array_equal(phi[0], phi[-1]), (group, name, k, "the duplicate pair differs")
        out[k] = (src, phi, its)
    src, phi, _ = out[64]
    one = eng.geodesic_solve(src[:1], TOL)[0]
    return out, one[0], phi[0]


# ------------------------------------------------------------------------------------------------------------ a. slab_gemm64
def _sentinel(shape, rng):
    """finite values, NaN, infinities and signed zeros in no regular pattern"""
    s = rng.normal(size=shape)
    flat = s.reshape(-1)
    flat[rng.permutation(flat.shape[0])[:flat.shape[0] // 3]] = np.nan
    flat[rng.permutation(flat.shape[0])[:flat.shape[0] // 9]] = -0.0
    flat[rng.permutation(flat.shape[0])[:flat.shape[0] // 11]] = np.inf
    return s


@pytest.mark.parametrize("Kc", (16, 32, 48, 64, 80, 144))
def test_slab_gemm64(Kc):
    rng = np.random.default_rng(Kc)
    eng = _engine()
    try:
        for M in (16, 32, 48):
            for nct in (1, 2, 3, 4, 0, 7):
                if nct in (0, 7) and M != 32:
                    continue
                w = 16 * min(max(nct, 1), 4)
                for alpha, beta in ((1.0, 0.0), (-1.0, 1.0)):
                    for lda in (Kc, Kc + 16):
                        A = np.full((M, lda), np.nan)
                        A[:, :Kc] = rng.normal(size=(M, Kc))
                        Z = np.full((Kc, 64), np.nan)
                        Z[:, :w] = rng.normal(size=(Kc, w))
                        out0 = _sentinel((M, 64), rng)
                        out0[:, :w] = np.nan if beta == 0.0 else rng.normal(size=(M, w))
                        got = eng.test_slab_gemm64(A, Z, out0.copy(), Kc, alpha, beta, nct)
                        where = "M=%d Kc=%d nct=%d alpha=%g beta=%g lda=%d" % (M, Kc, nct, alpha, beta, lda)
                        assert np.isfinite(got[:, :w]).all(), (where, "0 * NaN formed, or a column tile left out")
                        assert np.array_equal(got[:, w:].view(np.uint64), out0[:, w:].view(np.uint64)), (where, "columns >= 16 nct changed")
                        lo = gm.slab_gemm(A[:, :Kc], Z, out0, alpha, beta, nct, np.float64)
                        hi = gm.slab_gemm(A[:, :Kc], Z, out0, alpha, beta, nct, LD)
                        check("a gemm64", "out", got[:, :w], lo[:, :w], hi[:, :w], where)
        for M, K2 in ((24, 32), (32, 40), (8, 16)):
            with pytest.raises(RuntimeError, match="multiples of 16"):
                eng.test_slab_gemm64(np.zeros((M, K2)), np.zeros((K2, 64)), np.zeros((M, 64)), K2)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------ b. dense, batch
@pytest.mark.parametrize("name", gc.DENSE_CASES)
def test_dense_batch(name):
    eng = _engine()
    try:
        geo = _setup(eng, name, "dense")
        assert eng.geodesic_dense and "n_slabs" not in geo.__dict__
        _, one, of64 = _batches("b dense", eng, name, BATCHES_DENSE)
        same("b dense", one, of64, "%s batch of 1 vs batch of 64" % name)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------ c. dense, single
def _support_weight_cases(eng, phi, where):
    n = phi.shape[0]
    top = phi.max()
    for dmin, dmax in ((0.25 * top, 0.6 * top), (0.1 * top, 1.5 * top)):
        for v0, n_loc in ((0, n), (1, n - 1), (n // 2, n - n // 2), (n - 1, 1)):
            s = eng.test_support_weights(phi, v0, n_loc, dmin, dmax)
            hi = gm.support_weights(phi, v0, n_loc, dmin, dmax, LD)
            p = phi[v0:v0 + n_loc]
            assert s.shape == (n_loc,) and (s[p <= dmin] == 1.0).all() and (s[p >= dmax] == 0.0).all(), (where, v0, n_loc, "clamps")
            err = np.abs(s.astype(LD) - hi).max()
            assert err <= 4 * EPS, (where, v0, n_loc, dmin, dmax, float(err))
            seen = _SEEN.setdefault(("c single", "s (abs.)"), [0.0, 0.0, 4 * EPS])
            seen[0] = seen[1] = max(seen[0], float(err))
        if dmax < top:
            assert (phi >= dmax).any() and (phi <= dmin).any() and ((phi > dmin) & (phi < dmax)).any(), where


@pytest.mark.parametrize("name", gc.DENSE_CASES)
def test_dense_single_source_and_support_weights(name):
    n = gc.mesh(name)[0].shape[0]
    ref = gm.reference(name)
    interior = int(ref["src"][ref["src"].shape[0] // 2])
    assert 0 < interior < n - 1
    eng = _engine()
    try:
        _setup(eng, name, "dense")
        for s in (0, n - 1, interior):
            phi = eng.test_geodesic_field1(s)
            lo, hi = gm.rows(ref, "lo", [s])[0], gm.rows(ref, "hi", [s])[0]
            check("c single", "phi", phi, lo, hi, "%s source %d" % (name, s))
            batch = eng.geodesic_solve([s], TOL)[0][0]
            fro, mx = gm.deviation(phi, batch)
            b = max(FLOOR, MARGIN * max(gm.deviation(lo, hi)))
            print("c single %s source %d: single vs batch path %.2e / %.2e, bound %.2e" % (name, s, fro, mx, b))
            assert fro <= b and mx <= b
            assert phi.min() == 0.0
            _support_weight_cases(eng, phi, "%s source %d" % (name, s))
        with pytest.raises(RuntimeError, match="outside the mesh"):
            eng.test_geodesic_field1(n)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------ d. slab mode
def test_a_slab_case_grounds_a_vertex_inside_a_padded_slab():
    from animsnapbases_amd.geodesic import bfs_slabs
    ragged = []
    for name, target in gc.SLAB_CASES:
        ptr = bfs_slabs(gc.operators(name)[0], target)[1]
        if (ptr[-1] - ptr[-2]) % 16:
            ragged.append((name, target, int(ptr[-1] - ptr[-2])))
    print("grounded last vertex in a padded slab:", ragged)
    assert ragged
    assert bfs_slabs(gc.operators("n129")[0], 1)[1][1] == 1         # one vertex and 15 padding rows


@pytest.mark.parametrize("name,target", gc.SLAB_CASES)
def test_slab_mode(name, target, monkeypatch):
    eng = _engine()
    try:
        geo = _setup(eng, name, "slab", monkeypatch, target)
        assert geo.n_slabs == gc.SLAB_COUNTS[(name, target)], geo.n_slabs
        _, one, of64 = _batches("d slab", eng, name, BATCHES)
        same("d slab", one, of64, "%s target %d batch of 1 vs batch of 64" % (name, target))
        if (name, target) == ("n129", 40):          # the slab branch of asb_deflate_apply_geodesic: the batch solver with one source
            n = gc.mesh(name)[0].shape[0]
            phi = eng.test_geodesic_field1(n - 1)
            _check_fields("d slab", name, phi[None], [n - 1], "field1")
            assert np.array_equal(phi, eng.geodesic_solve([n - 1], TOL)[0][0])
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------ e. sparse mode
@pytest.mark.parametrize("name", gc.SPARSE_CG_CASES + gc.SPARSE_SWEEP_CASES)
def test_sparse_mode(name):
    ref = gm.reference(name)
    kw = dict(extra=ref["kappa"] * TOL, ceil=CEIL_SPARSE)
    eng = _engine()
    try:
        geo = _setup(eng, name, "pcg")
        assert not eng.geodesic_dense
        sweeps = name in gc.SPARSE_SWEEP_CASES
        if sweeps:
            assert geo.n_aggregates >= 1
            predicted = gc.jacobi_sweeps(gc.operators(name)[0])[2]
        else:
            assert "n_aggregates" not in geo.__dict__
        out, one, of64 = _batches("e sparse", eng, name, BATCHES, **kw)
        for k, (_, _, its) in out.items():
            print("e sparse %s nsrc=%d: %d heat %s, %d Poisson iterations" % (name, k, its[0], "sweeps" if sweeps else "iterations", its[1]))
            if sweeps:
                assert 0 < its[0] <= 2 * predicted, (name, k, its, predicted)
                assert 0 < its[1] < 400, (name, k, its)
        fro, mx = gm.deviation(one, of64)
        print("e sparse %s batch of 1 vs batch of 64: %s (%.2e / %.2e)" % (name, "bit-identical" if np.array_equal(one, of64) else
                                                                            "NOT bit-identical", fro, mx))
        b = max(FLOOR, kw["extra"])
        assert fro <= b and mx <= b
    finally:
        eng.close()


def test_sparse_solve_many_in_three_batches():
    name = "n600"
    ops = gc.operators(name)
    n = ops[0].shape[0]
    src = np.random.default_rng(130).permutation(n)[:130]
    hi = gm.HeatModel(*ops, dtype=LD).fields(src)
    lo = gm.HeatModel(*ops, dtype=np.float64).fields(src)
    kappa = gm.reference(name)["kappa"]
    eng = _engine()
    try:
        geo = _setup(eng, name, "pcg")
        phi = geo.solve_many(src)
        assert phi.shape == (130, n) and len(geo.last_iterations) == 3, geo.last_iterations
        for q in (0, 63, 64, 127, 128, 129):
            check("e sparse", "solve_many", phi[q], lo[q], hi[q], "%s row %d" % (name, q), extra=kappa * TOL, ceil=CEIL_SPARSE)
        check("e sparse", "solve_many", phi, lo, hi, "%s all 130" % name, extra=kappa * TOL, ceil=CEIL_SPARSE)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------ f. cache
def test_field_cache_slots():
    name = "tiny"
    n = gc.mesh(name)[0].shape[0]
    s60, s10 = np.arange(60) % n, (7 * np.arange(10) + 3) % n
    eng = _engine()
    try:
        _setup(eng, name, "dense")
        assert eng.geodesic_cache_add(s60) == list(range(60))
        assert eng.geodesic_cache_add(s10) == list(range(60, 70))           # crosses the 64-field slab boundary
        want = np.concatenate([eng.geodesic_solve(s60, TOL)[0], eng.geodesic_solve(s10, TOL)[0]])
        for slot in range(70):
            assert np.array_equal(eng.test_geodesic_cached(slot), want[slot]), slot
        for slot in (70, -1, 4096):
            with pytest.raises(RuntimeError, match="no cached field"):
                eng.test_geodesic_cached(slot)
        eng.geodesic_cache_clear()
        with pytest.raises(RuntimeError, match="no cached field"):
            eng.test_geodesic_cached(0)
        assert eng.geodesic_cache_add([n - 1]) == [0]
        assert np.array_equal(eng.test_geodesic_cached(0), eng.geodesic_solve([n - 1], TOL)[0][0])
        # fill it: 64 adds of 64
        eng.geodesic_cache_clear()
        full = (np.arange(64) * 3 + 1) % n
        for q in range(64):
            assert eng.geodesic_cache_add(full) == list(range(64 * q, 64 * q + 64))
        assert eng.GEODESIC_CACHE_SLOTS == 4096
        want = eng.geodesic_solve(full, TOL)[0]
        last = eng.test_geodesic_cached(4095)
        assert np.array_equal(last, want[63]) and np.array_equal(eng.test_geodesic_cached(64), want[0])
        with pytest.raises(RuntimeError, match="status -4.*cache is full"):
            eng.geodesic_cache_add([0])
        assert np.array_equal(eng.test_geodesic_cached(4095), last)         # nothing changed
        with pytest.raises(RuntimeError, match="no cached field"):
            eng.test_geodesic_cached(4096)
        _setup(eng, name, "dense")                                           # a new set-up empties the cache
        with pytest.raises(RuntimeError, match="no cached field"):
            eng.test_geodesic_cached(0)
        assert eng.geodesic_cache_add([0]) == [0]
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------ g. re-setup
RESETUP = (("n257", "dense", None), ("n129", "slab", 40), ("n600", "pcg", None), ("tiny", "dense", None), ("n257", "dense", None))


def _three_sources(name):
    n = gc.mesh(name)[0].shape[0]
    return np.array([0, int(gm.reference(name)["src"][5]), n - 1], dtype=np.int64)


def test_resetup_on_one_engine(monkeypatch):
    for name, backend, target in RESETUP:
        if (name, backend) not in _FRESH:
            eng = _engine()
            try:
                _setup(eng, name, backend, monkeypatch, target)
                _FRESH[(name, backend)] = eng.geodesic_solve(_three_sources(name), TOL)[0]
            finally:
                eng.close()
                monkeypatch.undo()
    eng = _engine()
    try:
        for step, (name, backend, target) in enumerate(RESETUP):
            geo = _setup(eng, name, backend, monkeypatch, target)
            monkeypatch.undo()
            assert eng.geodesic_dense == (backend != "pcg")
            src = _three_sources(name)
            phi = eng.geodesic_solve(src, TOL)[0]
            fresh = _FRESH[(name, backend)]
            where = "step %d: %s %s, re-used engine vs fresh engine" % (step, backend, name)
            if backend == "pcg":
                assert geo.n_aggregates >= 1
                kw = dict(extra=gm.reference(name)["kappa"] * TOL, ceil=CEIL_SPARSE)
                _check_fields("g re-setup", name, phi, src, "step %d" % step, **kw)
                fro, mx = gm.deviation(phi, fresh)
                print("g re-setup %s: %s (%.2e / %.2e)" % (where, "bit-identical" if np.array_equal(phi, fresh) else "NOT bit-identical",
                                                            fro, mx))
                assert fro <= max(FLOOR, kw["extra"]) and mx <= max(FLOOR, kw["extra"])
            else:
                _check_fields("g re-setup", name, phi, src, "step %d" % step)
                same("g re-setup", phi, fresh, where)
            if backend == "dense":                  # the single-source path reads the same state
                one = eng.test_geodesic_field1(int(src[1]))
                check("g re-setup", "field1", one, gm.rows(gm.reference(name), "lo", src[1:2])[0],
                      gm.rows(gm.reference(name), "hi", src[1:2])[0], where)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------ h. refusals
def test_host_side_refusals():
    from animsnapbases_amd.geodesic import coarse_operators, mesh_aggregates
    n = gc.mesh("tiny")[0].shape[0]
    eng = _engine()
    try:
        _setup(eng, "tiny", "dense")
        good = eng.geodesic_solve([0, n - 1], TOL)[0]
        with pytest.raises(RuntimeError, match="status -1"):
            eng.geodesic_solve(np.zeros(0, dtype=np.int64), TOL)
        with pytest.raises(RuntimeError, match="status -1"):
            eng.geodesic_solve(np.zeros(65, dtype=np.int64), TOL)
        for bad in (-1, n):
            with pytest.raises(RuntimeError, match="geodesic source %d outside the mesh" % bad):
                eng.geodesic_solve([0, bad, 1], TOL)
            with pytest.raises(RuntimeError, match="outside the mesh"):
                eng.geodesic_cache_add([bad])
        assert np.array_equal(eng.geodesic_solve([0, n - 1], TOL)[0], good)         # the refusals left the solver as it was
        # apply_geodesic: a mesh of another size than the snapshots'; the sparse mode
        X = np.random.default_rng(0).normal(size=(4, n + 1, 3))
        eng.upload(X, 0, n + 1)
        eng.deflate_begin(2, True)
        with pytest.raises(RuntimeError, match="the mesh has %d vertices, the snapshots %d" % (n, n + 1)):
            eng.apply_geodesic(0, 0.1, 0.3)
        _setup(eng, "n127", "pcg")
        with pytest.raises(RuntimeError, match="needs the dense or the slab geodesic backend"):
            eng.apply_geodesic(0, 0.1, 0.3)
        # coarse_setup: the damping of the heat sweeps must lie in (0, 1]
        A, L, G, D = gc.operators("n600")
        agg, nc = mesh_aggregates(A)
        Hc, Lc = coarse_operators(A, L, agg, nc)
        for omega in (0.0, 1.5):
            with pytest.raises(RuntimeError, match="damping .* not in"):
                eng.geodesic_setup(A, (-L).tocsr(), G, D, coarse=(agg, Hc, Lc, omega))
    finally:
        eng.close()
