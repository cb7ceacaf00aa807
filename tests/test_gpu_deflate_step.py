"""GPU (-m gpu): the greedy step of csrc/asb_kernels.h one kernel at a time -- k_stream, k_pick, k_local_best, k_block_argmax,
reduce_partials and the two 3 x 3 eigen-solvers on the device -- through the asb_test_* hooks of the step, against exact
references: integers (bit for bit), numpy.longdouble (forward bounds of a length-F sum) and mpmath (eigen-pairs, tolerances of
tests/eig3_cases.py).

Row lengths: one per (T, E2) configuration and both sides of every switch of pick_cfg and of the 16-frame padding.  Shard sizes
around the vertices-per-block count and around the grid cap (read from the hook, not assumed).  Left out for size, see
tests/README.md: at Fp = 32768 (0.79 MB per vertex and copy) the grid-stride case is a single run (F = 32753,
nblk_cap vpb + 1 + vpb vertices, one UPDATE pass); every other row length runs both cap-sized shards with two UPDATE passes.
"""
import itertools

import numpy as np
import pytest

import eig3_cases as ec
from animsnapbases_amd import _lib

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
FPS = (512, 528, 1024, 1040, 2048, 2064, 4096, 4112, 8192, 8208, 16384, 16400, 32768)
FS = (1, 2, 15, 16, 17) + tuple(f for Fp in FPS for f in (Fp - 15, Fp))
_CAP = []


def _cfg(F):
    out = np.zeros(5, dtype=np.int32)
    _lib.load().asb_test_pick_cfg((F + 15) // 16 * 16, out.ctypes.data)
    assert out[0] == 1
    return dict(T=int(out[1]), E2=int(out[2]), block=int(out[3]), vpb=int(out[4]))


def _engine(X, K, local=False, v0=0, n_loc=None):
    from animsnapbases_amd import HipEngine
    e = HipEngine(0)
    e.upload(X, v0, X.shape[1] if n_loc is None else n_loc)
    e.deflate_begin(K, local)
    return e


def _nblk_cap():
    if not _CAP:
        e = _engine(np.ones((1, 1, 3)), 1)
        _CAP.append(e.test_deflate_state()["nblk_cap"])
        e.close()
        assert _CAP[0] >= 8
    return _CAP[0]


def _shard_sizes(F):
    """(n_loc, UPDATE passes) for one row length"""
    Fp, vpb, cap = (F + 15) // 16 * 16, _cfg(F)["vpb"], _nblk_cap()
    small = {1, vpb - 1, vpb, vpb + 1, 300} - {0}
    out = [(n, 2) for n in sorted(small)]
    if Fp < 32768:
        out += [(cap * vpb - 1, 2), (cap * vpb + 1 + vpb, 2)]
    elif F != Fp:
        out += [(cap * vpb + 1 + vpb, 1)]
    return out


# ----------------------------------------------------------------------------------------------------------------------
# exact arithmetic: values are integers over a power-of-two denominator D, held in float64, computed in int64
# ----------------------------------------------------------------------------------------------------------------------
def _exact(v_int, D):
    """int64 numerators over D -> float64, asserting (on the reference alone) that every value is representable"""
    v_int = np.asarray(v_int)
    # below 2^53 every numerator AND every partial sum of non-negative ones is a float64 integer, in any order of summation
    assert np.abs(v_int).max(initial=0) < 1 << 53, "the reference needs more than 53 bits: not a fair bit-for-bit case"
    f = v_int.astype(np.float64)
    assert np.array_equal(f.astype(np.int64), v_int)
    return f / float(D)


def _ref_energy(Xr, D):
    """exact per-vertex sums of squares of Xr (n, 3, F), multiples of 1 / D: (float64, int numerators over D^2)"""
    n = Xr.shape[0]
    e = np.empty(n, dtype=np.int64)
    step = max(1, (1 << 22) // (3 * Xr.shape[2]))
    for a in range(0, n, step):
        Xi = np.rint(Xr[a:a + step] * float(D)).astype(np.int64)
        assert np.abs(Xi).max(initial=0) < 1 << 22
        e[a:a + step] = np.einsum("vdf,vdf->v", Xi, Xi)
    return _exact(e, D * D), e


def _ref_update(Xr, D, w, s4, m):
    """x -= w (w . x) s / 2^m in place on Xr, exactly; s4 = 4 s in {0, 1, 2, 4} or None (s = 1: two bits fewer in the
    denominator).  Returns (c (n, 3), new denominator)."""
    nz = np.flatnonzero(w)
    wz = w[nz].astype(np.int64)
    Xi = np.rint(Xr[:, :, nz] * float(D)).astype(np.int64)
    assert np.array_equal(Xi.astype(np.float64) / float(D), Xr[:, :, nz])
    assert (np.abs(Xi) * np.abs(wz)).sum(axis=2).max(initial=0) < 1 << 53          # signed partial sums of the dot products
    Ci = (Xi * wz).sum(axis=2)
    up = m
    if s4 is not None:
        Ci, up = Ci * s4[:, None].astype(np.int64), m + 2
    D2 = D << up
    Xr[:, :, nz] = _exact(Xi * (1 << up) - wz * Ci[:, :, None], D2)
    return _exact(Ci, D2), D2


def _check_records(st, e_ref, e_int, D2, vpb, cap):
    """every partial record of the last pass: block b holds the groups (v // vpb) % nblk == b"""
    n = e_ref.size
    nblk = min((n + vpb - 1) // vpb, cap)
    assert st["nblk"] == nblk and st["nblk_cap"] == cap
    assert np.array_equal(st["energy"], e_ref)
    blk = (np.arange(n) // vpb) % nblk
    order = np.lexsort((np.arange(n), -e_ref, blk))          # by block, then energy descending, then index
    first = order[np.r_[True, blk[order][1:] != blk[order][:-1]]]
    assert np.array_equal(blk[first], np.arange(nblk))
    assert np.array_equal(st["pidx"], first)
    assert np.array_equal(st["pmax"], e_ref[first])
    sums = np.zeros(nblk, dtype=np.int64)
    np.add.at(sums, blk, e_int)
    assert np.array_equal(st["psum"], _exact(sums, D2))
    tot_int = sum(int(x) for x in e_int)
    assert tot_int < 1 << 53, "the sum of the energies needs more than 53 bits: not a fair bit-for-bit case"
    tot = float(tot_int) / float(D2)
    assert float(np.sum(st["psum"])) == tot
    win = np.lexsort((st["pidx"], -st["pmax"]))[0]
    assert st["pidx"][win] == int(np.argmax(e_ref)) and st["pmax"][win] == e_ref.max()
    return tot


def _weight(rng, F, m):
    w = np.zeros(F)
    w[rng.choice(F, size=1 << m, replace=False)] = rng.choice([-1.0, 1.0], size=1 << m)
    return w


def _run_exact(F, n, passes, seed, Xv=None, s_all_one=False):
    """begin + `passes` UPDATE passes (with s, then without) on integer data; every value of every pass compared with ==.
    Returns the engine (open) and the exact residual."""
    rng = np.random.default_rng(seed)
    Fp, c, cap = (F + 15) // 16 * 16, _cfg(F), _nblk_cap()
    m = min(4, int(np.log2(F)))
    if Xv is None:
        Xv = rng.integers(-8, 9, size=(n, 3, F)).astype(np.float64)
    e = _engine(np.ascontiguousarray(Xv.transpose(2, 0, 1)), 2)
    D = 1
    Xr = Xv
    for k in range(-1, passes):
        if k >= 0:
            w = _weight(rng, F, m)
            s4 = None if (k == 1 or s_all_one) else rng.choice([0, 1, 2, 4], size=n)
            e.test_deflate_step(k, w, float(1 << m), None if s4 is None else s4 / 4.0)
            c_ref, D = _ref_update(Xr, D, w, s4, m)
        st = e.test_deflate_state(want_R=True, want_W=(k >= 0))
        e_ref, e_int = _ref_energy(Xr, D)
        tot = _check_records(st, e_ref, e_int, D * D, c["vpb"], cap)
        assert np.array_equal(st["R"][:, :, :F], Xr), (F, n, k)
        assert not st["R"][:, :, F:].any(), "padding of the residual"
        if k >= 0:
            assert np.array_equal(st["W"][k, :F], w) and not st["W"][k, F:].any()
            assert st["scal"][k, 1] == float(1 << m)
            r = e.results()
            assert np.array_equal(r["comps"][k], c_ref), (F, n, k)
            assert r["normR2_local"][k] == tot
        if n * Fp <= 1 << 22:
            assert np.array_equal(e.download_residual(), Xr.transpose(2, 0, 1))
    return e, Xr


@pytest.mark.parametrize("F", FS)
def test_stream_pass_exact_data_bit_for_bit(F):
    """k_stream<T, E2, false / true> on integer X, w in {-1, 0, 1} with 2^m non-zeros (|w|^2 = 2^m), s in {0, 1/4, 1/2, 1}: every
    product, quotient and sum is exactly representable whatever the order of the reduction and whether or not a product is fused
    into the sum (the reference asserts the 53 bits), so c_k, the residual with its padding, every energy, every partial record and
    the sum of the records are compared with ==.  Two UPDATE passes in a row: the second reads what the first wrote."""
    for i, (n, passes) in enumerate(_shard_sizes(F)):
        e, _ = _run_exact(F, n, passes, seed=1000 * F + i)
        e.close()


# ----------------------------------------------------------------------------------------------------------------------
# ties
# ----------------------------------------------------------------------------------------------------------------------
def _tie_sets(F, n):
    vpb, cap = _cfg(F)["vpb"], _nblk_cap()
    stride = cap * vpb
    sets = [("first and last", (0, n - 1)), ("two blocks", (5 * vpb, 9 * vpb + vpb - 1)),
            ("two rounds of the grid stride", (3 * vpb, 3 * vpb + stride)),
            ("block, round and last", (7 * vpb + vpb - 1, 2 * vpb + stride, n - 1))]
    if vpb > 1:
        sets.append(("two groups of one block", (11 * vpb, 11 * vpb + vpb - 1)))
        sets.append(("two groups of one block, second round", (stride + 4 * vpb + 1, stride + 4 * vpb)))
    return sets


@pytest.mark.parametrize("F", [24, 1000, 2048, 3000, 4100, 8200, 16500])          # one per k_stream configuration
def test_ties_take_the_lowest_index(F):
    """the maximal energy planted at two or three vertices (identical rows): groups of a block, blocks, rounds of the grid
    stride, first and last vertex.  The lowest index wins in the records of both kinds of pass, in k_pick and in k_local_best,
    before and after an UPDATE pass that keeps the rows tied."""
    vpb, cap = _cfg(F)["vpb"], _nblk_cap()
    n = cap * vpb + 13 * vpb + 1
    rng = np.random.default_rng(F)
    base = rng.integers(-4, 5, size=(n, 3, F)).astype(np.float64)
    plant = rng.choice([-9.0, 9.0], size=(3, F))
    for label, vs in _tie_sets(F, n):
        Xv = base.copy()
        Xv[list(vs)] = plant
        e, Xr = _run_exact(F, n, 0, seed=F, Xv=Xv)
        for k in (0, 1):
            en = (Xr ** 2).sum(axis=(1, 2))
            assert np.flatnonzero(en == en.max()).tolist() == sorted(vs), label          # the reference really ties, and only there
            rec = e.test_local_best(k)
            assert rec[0] == en.max() and int(rec[1:2].view(np.int64)[0]) == min(vs), label
            assert np.array_equal(rec[2:].reshape(3, -1)[:, :F], Xr[min(vs)]), label
            e.pick(k)
            assert e.get_pick(k)[0] == min(vs), label
            if k == 0:           # an UPDATE pass with s = 1: identical rows stay identical
                m = min(4, int(np.log2(F)))
                w = _weight(rng, F, m)
                e.test_deflate_step(0, w, float(1 << m))
                _ref_update(Xr, 1, w, None, m)
                st = e.test_deflate_state()
                win = np.lexsort((st["pidx"], -st["pmax"]))[0]
                assert st["pidx"][win] == min(vs), label
        e.close()


def _pick_state(e, k):
    st = e.test_deflate_state(want_W=True)
    return e.get_pick(k)[0], st["W"][k].copy(), st["scal"][k, 0], st["scal"][k, 1]


@pytest.mark.parametrize("F", [40, 2500])
def test_ties_across_shard_records_in_every_order(F):
    """three contexts as shards of one tensor, the maximum tied across shards: asb_deflate_pick over the three records in all
    six orders gives the lowest global index and W[k], sigma, |w|^2 bit-identical to the pick of one context holding the whole
    tensor (the record carries a copy of the slab, the kernel is the same)."""
    rng = np.random.default_rng(F + 1)
    N = 90
    cuts = [0, 31, 64, N]
    X = rng.integers(-4, 5, size=(F, N, 3)).astype(np.float64)
    plant = rng.integers(-9, 10, size=(F, 3)).astype(np.float64)
    plant[0] = 9
    for vs in ((40, 70), (5, 33, 89), (64, 88)):
        Xt = X.copy()
        Xt[:, list(vs)] = plant[:, None]
        whole = _engine(Xt, 1)
        whole.pick(0)
        want = _pick_state(whole, 0)
        whole.close()
        assert want[0] == min(vs)
        shards = [_engine(Xt, 1, v0=cuts[r], n_loc=cuts[r + 1] - cuts[r]) for r in range(3)]
        recs = np.stack([s.test_local_best(0) for s in shards])
        for r in range(3):
            mine = [v for v in vs if cuts[r] <= v < cuts[r + 1]]
            if mine:
                assert int(recs[r, 1:2].view(np.int64)[0]) == min(mine)
        for perm in itertools.permutations(range(3)):
            for s in shards[:2]:
                s.test_pick_records(0, recs[list(perm)])
                got = _pick_state(s, 0)
                assert got[0] == want[0], (vs, perm)
                assert np.array_equal(got[1], want[1]) and got[2] == want[2] and got[3] == want[3], (vs, perm)
        for s in shards:
            s.close()


def test_forced_row_owner_wins_others_abstain():
    rng = np.random.default_rng(77)
    F, N, cuts = 52, 60, [0, 20, 41, 60]
    X = rng.integers(-5, 6, size=(F, N, 3)).astype(np.float64)
    for g in (0, 19, 20, 47, 59):
        whole = _engine(X, 1)
        whole.force_next(g)
        whole.pick(0)
        want = _pick_state(whole, 0)
        whole.close()
        assert want[0] == g                                      # not the arg-max: the named row
        shards = [_engine(X, 1, v0=cuts[r], n_loc=cuts[r + 1] - cuts[r]) for r in range(3)]
        recs = []
        for s in shards:
            s.force_next(g)
            recs.append(s.test_local_best(0))
        recs = np.stack(recs)
        for r in range(3):
            if cuts[r] <= g < cuts[r + 1]:
                assert recs[r, 0] == 1.0e300 and int(recs[r, 1:2].view(np.int64)[0]) == g
                assert np.array_equal(recs[r, 2:].reshape(3, -1)[:, :F], X[:, g].T)         # the forced row's slab
            else:
                assert recs[r, 0] == -1.0
        for perm in ((0, 1, 2), (2, 1, 0), (1, 2, 0)):
            shards[1].test_pick_records(0, recs[list(perm)])
            got = _pick_state(shards[1], 0)
            assert got[0] == g and np.array_equal(got[1], want[1]) and got[2] == want[2] and got[3] == want[3]
        for s in shards:
            s.close()


# ----------------------------------------------------------------------------------------------------------------------
# float data: forward bounds of a length-F sum in any order
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", ["normal", "uniform"])
@pytest.mark.parametrize("F", FS)
def test_stream_pass_float_data_forward_bounds(F, dist):
    """|c - c_ref| <= 2 (F + 2) eps sum|x||w| |s| / wn2;  |x' - x'_ref| <= eps (|x| + 2 |w| |c_ref|) + |w| dc;
    |e - e_ref| <= (3 F + 4) eps e_ref + 2 sqrt(e_ref) |dx'|_2 + |dx'|_2^2, with dc, dx' the bounds themselves; reference in
    numpy.longdouble.  Per-vertex scales over 1e-6 .. 1e6.  Component 0 is a real step -- asb_deflate_pick's own W[0] and |w|^2,
    read back, then asb_deflate_apply with s --, component 1 a caller's random w without s."""
    ld = np.longdouble
    assert np.finfo(ld).eps < 1e-18
    rng = np.random.default_rng(7 * F + (dist == "normal"))
    n = 29
    Xv = (rng.normal(size=(n, 3, F)) if dist == "normal" else rng.uniform(-1, 1, size=(n, 3, F)))
    Xv *= 10.0 ** rng.uniform(-6, 6, size=(n, 1, 1))
    e = _engine(np.ascontiguousarray(Xv.transpose(2, 0, 1)), 2)
    Xr = Xv.astype(ld)
    bound_x = np.zeros((n, 3, F), dtype=ld)
    for k in range(-1, 2):
        if k >= 0:
            X_in = e.test_deflate_state(want_R=True)["R"][:, :, :F]          # what the pass reads: the device's own residual
            if k == 0:
                e.pick(0)
                st = e.test_deflate_state(want_W=True)
                w, wn2 = st["W"][0, :F].copy(), float(st["scal"][0, 1])
                assert not st["W"][0, F:].any() and abs(wn2 - float((w.astype(ld) ** 2).sum())) <= (F + 2) * EPS * wn2
                s = rng.uniform(0, 1, size=n)
                s[::7] = 0.0
                s[3::7] = 1.0
                e.apply(0, s)
            else:
                w = rng.uniform(-1, 1, size=F)
                wn2, s = float((w ** 2).sum()), None
                e.test_deflate_step(k, w, wn2, s)
            sv = (np.ones(n) if s is None else s).astype(ld)
            xin, wl = X_in.astype(ld), w.astype(ld)
            c_ref = (xin @ wl) * sv[:, None] / ld(wn2)
            bound_c = 2 * (F + 2) * EPS * (np.abs(xin) @ np.abs(wl)) * sv[:, None] / ld(wn2)
            Xr = xin - wl * c_ref[:, :, None]
            bound_x = EPS * (np.abs(xin) + 2 * np.abs(wl) * np.abs(c_ref)[:, :, None]) + np.abs(wl) * bound_c[:, :, None]
            c = e.results()["comps"][k]
            assert (np.abs(c.astype(ld) - c_ref) <= bound_c).all(), (F, k, float((np.abs(c - c_ref) / (bound_c + 1e-300)).max()))
        st = e.test_deflate_state(want_R=True)
        assert (np.abs(st["R"][:, :, :F].astype(ld) - Xr) <= bound_x).all(), (F, k)
        assert not st["R"][:, :, F:].any()
        e_ref = (Xr ** 2).sum(axis=(1, 2))
        dx = np.sqrt((bound_x ** 2).sum(axis=(1, 2)))
        bound_e = (3 * F + 4) * EPS * e_ref + 2 * np.sqrt(e_ref) * dx + dx ** 2
        assert (np.abs(st["energy"].astype(ld) - e_ref) <= bound_e).all(), (F, k)
        # the records hold the energies just checked: winner and sum
        win = np.lexsort((st["pidx"], -st["pmax"]))[0]
        assert st["pidx"][win] == int(np.argmax(st["energy"])) and st["pmax"][win] == st["energy"].max()
        assert abs(st["psum"].sum() - st["energy"].sum()) <= n * EPS * st["energy"].sum()
    e.close()


# ----------------------------------------------------------------------------------------------------------------------
# k_pick: sigma, w, |w|^2 of the chosen slab
# ----------------------------------------------------------------------------------------------------------------------
def _slabs(F, rng):
    t = 2 * np.pi * np.arange(F) / F
    gen = rng.normal(size=(3, F)) * np.array([[3.0], [1.0], [0.2]])
    line = np.outer([2.0, -3.0, 6.0], rng.integers(-9, 10, size=F).astype(np.float64))
    line[:, 0] = [2.0, -3.0, 6.0]
    circle = _orth(rng) @ np.stack([np.cos(t), np.sin(t), 0.25 * np.cos(3 * t)])
    out = [("generic", "gram", gen), ("line", "rank12", line), ("circle", "double", circle), ("zero", "zero", np.zeros((3, F)))]
    for sc in (1e-120, 1e120):
        out += [("generic*%g" % sc, "gram", gen * sc), ("line*%g" % sc, "rank12", line * sc), ("circle*%g" % sc, "double", circle * sc)]
    return out


def _gram_depth(F):
    """roundings a term of k_pick's Gram sums passes through at most (see test_pick_values_against_svd_reference)"""
    return (F + 255) // 256 + 12


def _orth(rng):
    Q, R = np.linalg.qr(rng.normal(size=(3, 3)))
    return Q * np.sign(np.diag(R))


@pytest.mark.parametrize("F", [64, 1000])
def test_pick_values_against_svd_reference(F):
    """sigma, w = sigma_1 Vt[0] (up to sign) and |w|^2 of k_pick for slabs of the eigen-families: motion in general position, on a
    line (rank 1), on a circle (double top singular value), no motion at all, and times 1e-120 / 1e120.  Reference: the Gram
    matrix summed in numpy.longdouble, its eigen-pairs at 60 digits.  Tolerances: the constants of tests/eig3_cases.py for the
    3 x 3 solve, plus the forward bound of the f64 Gram sums that feed it in the shape k_pick sums them (256 threads of
    ceil(F / 256) terms each, a 6-level wave butterfly, 4 waves in sequence: every term passes through at most
    ceil(F / 256) + 11 roundings), dG = max_ij (ceil(F / 256) + 12) eps sum_f |s_if| |s_jf| (a symmetric perturbation of norm
    <= 3 dG: lambda moves by that much, the direction by that over the gap)."""
    import mpmath as mp
    ld = np.longdouble
    rng = np.random.default_rng(F)
    slabs = _slabs(F, rng)
    X = np.stack([s for _, _, s in slabs]).transpose(2, 0, 1)            # (F, n, 3)
    e = _engine(np.ascontiguousarray(X), len(slabs))
    for v, (label, fam, S) in enumerate(slabs):
        e.force_next(v)
        e.pick(v)
        idx, w, sigma, wn2 = _pick_state(e, v)
        assert idx == v and np.isfinite(w).all() and np.isfinite([sigma, wn2]).all(), label
        assert not w[F:].any(), label
        w = w[:F]
        if fam == "zero":
            assert sigma == 0.0 and wn2 == 0.0 and not w.any()
            continue
        Sl = S.astype(ld)
        a6 = ec.a6_of((Sl @ Sl.T).astype(np.float64))
        ref = ec.reference(a6)
        dG = float(_gram_depth(F) * EPS * (np.abs(Sl) @ np.abs(Sl).T).max()) + 2 * EPS * ref["sc"]          # + rounding of a6 itself
        b = ec.bounds(fam)
        lam = float(ref["lam"][0])
        tol_lam = b["lam"] * EPS * ref["sc"] + 3 * dG
        assert abs(sigma * sigma - lam) <= tol_lam + 4 * EPS * lam, (label, sigma * sigma, lam)
        assert abs(wn2 - lam) <= tol_lam + (F + 16) * EPS * lam, (label, wn2, lam)            # |u^T S|^2 = lambda_1
        cl = ec.cluster_of(ref)
        vecs = [np.array([float(x) for x in ref["vecs"][i]]) for i in cl]
        gap = float(ref["lam"][0] - ref["lam"][len(cl)])
        theta = (b["ang" if len(cl) == 1 else "sub"] * EPS * ref["sc"] + 3 * dG) / gap
        # w = u^T S with u within theta of the top eigen-space: what is left of w after removing span{v_i^T S} is d^T S with
        # |d| <= theta, plus the rounding of the three-term products
        P = np.stack([vv @ S for vv in vecs])                              # (|cl|, F), rows orthogonal: v_i^T G v_j = 0
        coef = [(w @ p) / (p @ p) for p in P]
        rest = w - sum(c * p for c, p in zip(coef, P))
        assert np.linalg.norm(rest) <= (theta + 8 * EPS) * np.linalg.norm(S), (label, float(np.linalg.norm(rest)))
        if len(cl) == 1:
            assert abs(abs(coef[0]) - 1) <= theta + 8 * EPS + tol_lam / lam, (label, coef)
    e.close()


def test_pick_local_mode_projection_branches():
    """support='local': the +-projection test of k_pick on exact slabs (motion along x, u = e_0, w = the integer row): a generic
    row, projections of equal norm (the negative branch, as the oracle's `pos if norm(pos) > norm(neg) else neg`), a row without
    positive and one without negative entries, the zero slab; and a random slab against the oracle's rule applied to the
    reference's w."""
    from fractions import Fraction
    from oracle.asb_oracle import project_weight
    rng = np.random.default_rng(3)
    F = 300
    rows = [rng.integers(-9, 10, size=F).astype(np.float64)]
    half = rng.integers(1, 10, size=F // 2).astype(np.float64)
    rows.append(np.stack([half, -half], axis=1).reshape(-1))               # (a, -a, b, -b, ..): equal norms, equal maxima
    rows.append(-rng.integers(0, 10, size=F).astype(np.float64))           # no positive entry
    rows.append(rng.integers(0, 10, size=F).astype(np.float64))            # no negative entry
    rows.append(np.zeros(F))
    gen = rng.normal(size=(3, F)) * np.array([[3.0], [1.0], [0.2]])
    n = len(rows) + 1
    X = np.zeros((F, n, 3))
    for v, r in enumerate(rows):
        X[:, v, 0] = r
    X[:, n - 1] = gen.T
    e = _engine(X, n, local=True)
    for v in range(n):
        e.force_next(v)
        e.pick(v)
        idx, w, sigma, wn2 = _pick_state(e, v)
        assert idx == v and not w[F:].any() and np.isfinite(w).all()
        w = w[:F]
        assert (w >= 0).all()
        if v < len(rows):
            pos, neg = project_weight(rows[v]), project_weight(-rows[v])
            # the oracle's `pos if norm(pos) > norm(neg) else neg`, decided in exact arithmetic (integers over their maxima)
            npos2 = Fraction(int((np.maximum(rows[v], 0) ** 2).sum()), max(int(rows[v].max()), 1) ** 2)
            nneg2 = Fraction(int((np.maximum(-rows[v], 0) ** 2).sum()), max(int((-rows[v]).max()), 1) ** 2)
            want = pos if npos2 > nneg2 else neg
            assert np.array_equal(w, want), v                                # integers over their maximum: one rounding, the same
            assert abs(wn2 - (w ** 2).sum()) <= (F + 2) * EPS * wn2
            assert sigma == np.sqrt((rows[v] ** 2).sum())
            if v == 1:
                assert npos2 == nneg2 and np.array_equal(want, neg) and not np.array_equal(pos, neg)
        else:
            # reference: 60-digit top eigenvector of the slab's Gram matrix (summed in longdouble), w0 = u_ref^T S, the oracle's
            # rule on +-w0.  The kernel's u is within theta of u_ref (constants of tests/eig3_cases.py + the Gram sums' forward
            # bound, as in test_pick_values_against_svd_reference), so every entry of u^T S is within (theta + 8 eps) |S_f| of
            # w0's and the scale max(w0) by as much; after the division by the scale: twice that, relative to the scale.
            Sl = gen.astype(np.longdouble)
            ref = ec.reference(ec.a6_of((Sl @ Sl.T).astype(np.float64)))
            assert len(ec.cluster_of(ref)) == 1
            dG = float(_gram_depth(F) * EPS * (np.abs(Sl) @ np.abs(Sl).T).max()) + 2 * EPS * ref["sc"]
            theta = (ec.bounds("gram")["ang"] * EPS * ref["sc"] + 3 * dG) / float(ref["lam"][0] - ref["lam"][1])
            w0 = np.array([float(x) for x in ref["vecs"][0]]) @ gen
            pos, neg = project_weight(w0), project_weight(-w0)
            want = pos if np.linalg.norm(pos) > np.linalg.norm(neg) else neg
            assert abs(np.linalg.norm(pos) - np.linalg.norm(neg)) > 1e-6          # the branch is not a matter of rounding
            scale = (-w0).max() if want is neg else w0.max()
            tol = 2 * (theta + 8 * EPS) * np.sqrt((gen ** 2).sum(axis=0)).max() / scale + 4 * EPS
            assert w.max() == 1.0 and np.abs(w - want).max() <= tol, (float(np.abs(w - want).max()), tol)
    e.close()


# ----------------------------------------------------------------------------------------------------------------------
# k_block_argmax
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_block_argmax_exact_energies(p):
    """asb_deflate_block_argmax on integer energies (F = 1: energy = x^2): random small sums (many ties) and a planted maximum at
    two or three blocks -- neighbouring threads, two blocks of the grid, two rounds of its 65 536-block stride -- on a shard that
    starts at v0 > 0 (global block index); a shard that does not hold whole blocks is refused."""
    rng = np.random.default_rng(p)
    for nb in (1, 255, 256, 257, 65535, 65536, 65537 + 256):
        n, v0 = nb * p, 7 * p
        N = v0 + n + 3
        grid = min((nb + 255) // 256, 256)
        plants = [(), (nb - 1,), (min(3, nb - 1), min(4, nb - 1)), (min(10, nb - 1), min(10 + 256, nb - 1), nb - 1)]
        if nb > grid * 256:
            plants += [(5, 5 + grid * 256), (grid * 256 + 2, 300)]
        for pl in plants:
            X = np.zeros((1, N, 3))
            X[0, :, 0] = rng.integers(0, 4, size=N)
            X[0, :, 2] = rng.integers(0, 2, size=N)
            for b in pl:
                X[0, v0 + b * p:v0 + (b + 1) * p] = [0.0, 100.0, 0.0]          # exactly tied block sums
            e = _engine(X, 1, v0=v0, n_loc=n)
            en = (X[0, v0:v0 + n] ** 2).sum(axis=1)
            assert np.array_equal(e.test_deflate_state()["energy"], en)
            sums = en.reshape(nb, p).sum(axis=1)
            blk, val = e.block_argmax(p)
            assert blk == 7 + int(np.argmax(sums)) and val == sums.max(), (p, nb, pl)
            if pl:
                assert blk == 7 + min(pl) and np.flatnonzero(sums == sums.max()).tolist() == sorted(set(pl))
            e.close()
    X = np.ones((1, 40, 3))
    for v0, n in ((0, 4 * p + 1), (1, 4 * p)):
        if p == 1:
            continue
        e = _engine(X, 1, v0=v0, n_loc=n)
        with pytest.raises(RuntimeError, match="whole blocks"):
            e.block_argmax(p)
        e.close()


# ----------------------------------------------------------------------------------------------------------------------
# the eigen-solvers on the device
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eig_cases():
    return [(fam, label, a6, ec.reference(a6)) for fam, label, a6 in ec.all_cases()]


@pytest.mark.parametrize("fast", [False, True])
def test_eig3_solvers_on_the_device(fast, eig_cases):
    """the whole CPU family through the device (its own cos / acos / sqrt / divide): same checks, same constants; device and host
    results of the same solver agree to the same bounds (not bit for bit)."""
    from animsnapbases_amd import HipEngine
    e = HipEngine(0)
    A = np.stack([a6 for _, _, a6, _ in eig_cases])
    out = e.test_eig3_dev(A, fast)
    e.close()
    lib = _lib.load()
    who = "device eig3_top_fast" if fast else "device eig3_top"
    for (fam, label, a6, ref), o in zip(eig_cases, out):
        ec.check_case(fam, label, a6, o, ref, who)
        if fam == "zero":
            continue
        h = np.zeros(4)
        a = np.ascontiguousarray(a6)
        (lib.asb_test_eig3_fast if fast else lib.asb_test_eig3)(a.ctypes.data, h.ctypes.data)
        b = ec.bounds(fam)
        assert abs(o[0] - h[0]) <= 2 * b["lam"] * EPS * ref["sc"], label
        if len(ec.cluster_of(ref)) == 1 and not ec.sign_skipped(ref):
            gap = float(ref["lam"][0] - ref["lam"][1])
            assert np.abs(o[1:] - h[1:]).max() <= 2 * b["ang"] * EPS * ref["sc"] / gap + 4 * EPS, label


# ----------------------------------------------------------------------------------------------------------------------
# the limit
# ----------------------------------------------------------------------------------------------------------------------
def test_frame_limit_refused_and_context_survives():
    """F = 32768 runs (the parametrised tests above); F = 32769 is refused by both uploads with ASB_ERR_LIMIT and a message naming
    the limit, and the context works afterwards."""
    from animsnapbases_amd import HipEngine
    e = HipEngine(0)
    X = np.zeros((32769, 2, 3))
    with pytest.raises(RuntimeError, match=r"status %d: .*32768" % _lib.ERR_LIMIT):
        e.upload(X, 0, 2)
    with pytest.raises(RuntimeError, match=r"status %d: .*32768" % _lib.ERR_LIMIT):
        e.upload_rest(X, 0, 2, None, 0, True)
    # one real pick + apply step at the limit, bit for bit: the winner moves along x with a row b in {-1, 0, 1} of 64 non-zeros
    # (Gram matrix diag(64, 0, 0): u = e_0, w = b, |w|^2 = 64, sigma = 8 exactly); the others are sparse small integers of less
    # energy; s in {0, 1/4, 1/2, 1}
    rng = np.random.default_rng(0)
    F, n, win, m = 32768, 300, 211, 6
    Xv = np.zeros((n, 3, F))
    for v in range(n):
        for d in range(3):
            Xv[v, d, rng.choice(F, size=4, replace=False)] = rng.choice([-2.0, -1.0, 1.0, 2.0], size=4)
    b = _weight(rng, F, m)
    Xv[win] = 0.0
    Xv[win, 0] = b
    e.upload(np.ascontiguousarray(Xv.transpose(2, 0, 1)), 0, n)
    e.deflate_begin(2, False)
    e.pick(0)
    st = e.test_deflate_state(want_W=True)
    assert e.get_pick(0)[0] == win and np.array_equal(st["W"][0], b) and st["scal"][0, 1] == 64.0 and st["scal"][0, 0] == 8.0
    s4 = rng.choice([0, 1, 2, 4], size=n)
    s4[win] = 4
    e.apply(0, s4 / 4.0)
    c_ref, D = _ref_update(Xv, 1, b, s4, m)
    st = e.test_deflate_state(want_R=True)
    e_ref, e_int = _ref_energy(Xv, D)
    _check_records(st, e_ref, e_int, D * D, _cfg(F)["vpb"], st["nblk_cap"])
    assert np.array_equal(st["R"], Xv) and e_ref[win] == 0.0
    assert np.array_equal(e.results()["comps"][0], c_ref)
    e.close()
