"""GPU (-m gpu): the expansion q~ = o + U z fused with the difference metrics (``asb_gsub_expand_diff``, csrc/asb_zroll.hip,
DESIGN.md 3.23), through ``eng.gsub_expand_diff``.  Every measured err / bound is printed; no frame or case is left out.

1. Exact zeros.  Chains N in ``CHAINS`` (the edges of the 32-vertex tile), r in ``RS`` and N, widths ``WIDTHS``: with
   a := ``gsub_expand(z)`` downloaded and uploaded again, every sum of squared differences and max |e| is exactly 0.0, in total and
   per frame (q~ is ``gsub_expand``'s bit for bit).  The norms against longdouble sums of a^2: (3 N + 16) eps per frame and
   (N F' + 16) eps per axis in total, relative -- sums of non-negative terms in ANY fixed order of at most that many terms (the
   three axis sums of a frame are added on the host: two of the 16).  The signed max is a.max() exactly.
2. One entry moved: delta added to a[f*, v*, d*] for v* in {0, 15, 16, 31, 32, N - 1}, f* in {0, 63, 64, w - 1} (those inside the
   tensor) and every d*.  Axis d* of the totals and frame f* of the per-frame sums are fl(fl(a' - q~)^2) exactly -- one non-zero
   term, fma onto 0 rounds once, as the host's product does --, everything else 0.0, max |e| = |fl(a' - q~)|.
3. General a (entries scaled by 10^+-2 per vertex) against the longdouble model of e = a - q~, q~ the downloaded expansion: the
   sums within the bounds of 1. (the rounding of e itself is one of the 16), both maxima exact, the records of the first w frames
   bit-identical across widths, two calls bit-identical, ``force_diff(a, gsub_expand(z))`` with the same maxima and sums within
   the sum of both bounds, a NaN in one entry of a in that frame's and that axis's sums and in no other frame's.
4. Refusals: no subspace held, n_frames < 1, null pointers.
5. A chain of 8 225 vertices (258 tiles: two per block, 129 groups): 1. and 3. where a block walks more than one tile.

Largest err / bound measured on an MI355X: 1. norms 0.048 (chain 2); 2. 4 572 cases, all exact; 3. 0.056 (chain 2); 5. 4.0e-4 (also in
DESIGN.md 3.23)."""
import ctypes

import numpy as np
import pytest

from gslab_model import chain_matrix
from gsub_model import EPS, LD
from test_gpu_gsub import CHAINS, RS, WIDTHS, _snaps

pytestmark = pytest.mark.gpu


def _dev(eng, a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:%d" % eng.device_id)


def _expand(eng, zd, n):
    import torch
    q = torch.full((zd.shape[0], n, 3), float("nan"), dtype=torch.float64, device=zd.device)
    eng.gsub_expand(zd.data_ptr(), zd.shape[0], q.data_ptr())
    return q


def _chain(n, seed):
    """(engine, rng, r -> the subspace of r components set up on the device) for the chain of n vertices."""
    from animsnapbases_amd import projections as proj
    rng = np.random.default_rng(seed + n)
    A = chain_matrix(n)
    eng = _snaps(rng.standard_normal((2, n, 3)))._engine
    comps, origin = rng.standard_normal((max(min(n, max(RS)), 1) if n > 65 else n, n, 3)), rng.standard_normal((n, 3))
    return eng, rng, lambda r: eng.gsub_setup(A, proj.subspace_basis(comps, r), origin)


def _ranks(n):
    return sorted(set(k for k in RS + [n] if k <= n))


def _sum_ratios(a, e, sums, norms, pf):
    """The largest err / bound of the sums against the longdouble sums of e^2 (None: exact zeros are checked elsewhere) and a^2."""
    w, n = a.shape[:2]
    a2 = a.astype(LD) ** 2
    worst = 0.0
    pairs = [(norms[:3], a2.sum(axis=(0, 1)), n * w + 16), (pf[:, 1], a2.sum(axis=(1, 2)), 3 * n + 16)]
    if e is not None:
        e2 = e.astype(LD) ** 2
        pairs += [(sums, e2.sum(axis=(0, 1)), n * w + 16), (pf[:, 0], e2.sum(axis=(1, 2)), 3 * n + 16)]
    for got, ref, terms in pairs:
        err, bnd = np.abs(got - ref).astype(np.float64), (terms * EPS * ref).astype(np.float64)
        assert (err <= bnd).all(), (w, n, terms, float((err / np.maximum(bnd, 1e-300)).max()))
        if (bnd > 0).any():
            worst = max(worst, float((err[bnd > 0] / bnd[bnd > 0]).max()))
    return worst


# ------------------------------------------------------------------ 1. exact zeros
def _check_zeros(eng, n, r, w, zin):
    zd = _dev(eng, zin[:w])
    a = _expand(eng, zd, n).cpu().numpy()
    assert np.isfinite(a).all()
    ad = _dev(eng, a)                                                                       # downloaded and uploaded again
    sums, mx, norms, pf = eng.gsub_expand_diff(ad.data_ptr(), zd.data_ptr(), w, True)
    assert pf.shape == (w, 2)
    assert (sums == 0.0).all() and mx == 0.0 and (pf[:, 0] == 0.0).all(), (n, r, w, sums, mx)
    assert norms[3] == a.max()
    return _sum_ratios(a, None, sums, norms, pf)


@pytest.mark.parametrize("n", CHAINS)
def test_exact_zeros_on_the_expansion_itself(n):
    eng, rng, setup = _chain(n, 900)
    worst = 0.0
    for r in _ranks(n):
        setup(r)
        zin = rng.standard_normal((max(WIDTHS), r, 3))
        for w in WIDTHS:
            worst = max(worst, _check_zeros(eng, n, r, w, zin))
    print("chain %d exact zeros; norms: largest err / bound %.3g" % (n, worst))
    assert worst < 1.0


# ------------------------------------------------------------------ 2. one entry moved
@pytest.mark.parametrize("n", CHAINS)
def test_one_entry_moved(n):
    eng, rng, setup = _chain(n, 1000)
    count = 0
    for r in _ranks(n):
        setup(r)
        zin = rng.standard_normal((max(WIDTHS), r, 3))
        for w in WIDTHS:
            zd = _dev(eng, zin[:w])
            ad = _expand(eng, zd, n)
            q = ad.cpu().numpy()
            for fs in sorted(set(f for f in (0, 63, 64, w - 1) if 0 <= f < w)):
                for vs in sorted(set(v for v in (0, 15, 16, 31, 32, n - 1) if 0 <= v < n)):
                    for ds in range(3):
                        delta = float(rng.standard_normal() * 10.0 ** rng.integers(-2, 3))
                        moved = q[fs, vs, ds] + delta                                       # fl(a + delta), as the device holds it
                        ad[fs, vs, ds] = moved
                        sums, mx, norms, pf = eng.gsub_expand_diff(ad.data_ptr(), zd.data_ptr(), w, True)
                        ad[fs, vs, ds] = q[fs, vs, ds]
                        e = moved - q[fs, vs, ds]
                        assert e != 0.0
                        want = np.zeros(3)
                        want[ds] = e * e
                        wf = np.zeros(w)
                        wf[fs] = e * e
                        assert np.array_equal(sums, want) and np.array_equal(pf[:, 0], wf) and mx == abs(e), (n, r, w, fs, vs, ds, sums, e * e, mx)
                        count += 1
    print("chain %d one entry moved: %d cases, every sum and max exact" % (n, count))


# ------------------------------------------------------------------ 3. general a
def _check_general(eng, n, r, rng, widths):
    W = max(widths)
    zin = rng.standard_normal((W, r, 3))
    x = rng.standard_normal((W, n, 3)) * 10.0 ** rng.integers(-2, 3, size=(1, n, 1))
    worst, wide = 0.0, None
    for w in sorted(widths, reverse=True):
        zd, ad = _dev(eng, zin[:w]), _dev(eng, x[:w])
        qd = _expand(eng, zd, n)
        q, a = qd.cpu().numpy(), x[:w]
        got = eng.gsub_expand_diff(ad.data_ptr(), zd.data_ptr(), w, True)
        sums, mx, norms, pf = got
        worst = max(worst, _sum_ratios(a, a.astype(LD) - q.astype(LD), sums, norms, pf))
        assert mx == np.abs(a - q).max() and norms[3] == a.max()                            # both maxima exact
        again = eng.gsub_expand_diff(ad.data_ptr(), zd.data_ptr(), w, True)                 # two calls: identical bits
        assert np.array_equal(again[0], sums) and again[1] == mx and np.array_equal(again[2], norms) and np.array_equal(again[3], pf)
        if wide is None:
            wide = pf
        assert np.array_equal(pf, wide[:w])                                                 # a frame's record does not depend on the width
        # the parent's two calls: the same maxima, sums within both bounds
        fs, fm, fn, fpf = eng.force_diff(ad.data_ptr(), qd.data_ptr(), w, n, True)
        assert fm == mx and fn[3] == norms[3]
        for mine, theirs, terms in ((sums, fs, n * w + 16), (norms[:3], fn[:3], n * w + 16), (pf[:, 0], fpf[:, 0], 3 * n + 16), (pf[:, 1], fpf[:, 1], 3 * n + 16)):
            err, bnd = np.abs(mine - theirs), 2.0 * terms * EPS * np.maximum(mine, theirs)
            assert (err <= bnd).all()
            worst = max(worst, float((err / bnd).max()))
        # a NaN in one entry: that frame's and that axis's sums, no other frame's
        f0, v0, d0 = w // 2, (5 * n) // 7, 1
        keep = float(ad[f0, v0, d0])
        ad[f0, v0, d0] = float("nan")
        ns, nm, nn, npf = eng.gsub_expand_diff(ad.data_ptr(), zd.data_ptr(), w, True)
        ad[f0, v0, d0] = keep
        others = np.arange(w) != f0
        assert np.isnan(npf[f0]).all() and np.array_equal(npf[others], pf[others])
        assert np.isnan(ns[d0]) and np.isnan(nn[d0])
        for d in (0, 2):
            assert ns[d] == sums[d] and nn[d] == norms[d]
    return worst


@pytest.mark.parametrize("n", CHAINS)
def test_general_tensors_against_the_longdouble_model(n):
    eng, rng, setup = _chain(n, 1100)
    worst = 0.0
    for r in _ranks(n):
        setup(r)
        worst = max(worst, _check_general(eng, n, r, rng, WIDTHS))
    print("chain %d general a: largest err / bound %.3g" % (n, worst))
    assert worst < 1.0


# ------------------------------------------------------------------ 4. refusals
def test_refusals_and_error_codes():
    import torch
    from animsnapbases_amd import _lib
    V = ctypes.c_void_p
    n, r, w = 17, 4, 5
    eng, rng, setup = _chain(n, 1200)
    dev = "cuda:%d" % eng.device_id
    a, z = torch.zeros((w, n, 3), dtype=torch.float64, device=dev), torch.zeros((w, r, 3), dtype=torch.float64, device=dev)
    out = np.zeros(4)
    call = lambda *args: eng.lib.asb_gsub_expand_diff(eng.h, *args, _lib.ptr(out), None, None, None)
    # no subspace held: the error of asb_gsub_expand
    assert call(V(a.data_ptr()), V(z.data_ptr()), w) == _lib.ERR_ARG and b"no position subspace" in eng.lib.asb_last_error(eng.h)
    with pytest.raises(RuntimeError, match="no position subspace"):
        eng.gsub_expand_diff(a.data_ptr(), z.data_ptr(), w)
    setup(r)
    # counts before pointers, then the pointers
    assert call(V(1), V(1), 0) == _lib.ERR_ARG and call(V(1), V(1), -3) == _lib.ERR_ARG
    assert call(None, V(z.data_ptr()), w) == _lib.ERR_ARG and call(V(a.data_ptr()), None, w) == _lib.ERR_ARG
    assert eng.lib.asb_gsub_expand_diff(None, V(a.data_ptr()), V(z.data_ptr()), w, None, None, None, None) == _lib.ERR_ARG
    assert call(V(1), V(1), 65535 * 64 + 1) == _lib.ERR_LIMIT                                 # the frame limit of asb_gsub_expand
    # every output pointer may be NULL; the engine is usable afterwards
    assert eng.lib.asb_gsub_expand_diff(eng.h, V(a.data_ptr()), V(z.data_ptr()), w, None, None, None, None) == 0
    sums, mx, norms, pf = eng.gsub_expand_diff(a.data_ptr(), z.data_ptr(), w)
    assert pf is None and np.isfinite(sums).all() and np.isfinite(norms[:3]).all()


# ------------------------------------------------------------------ 5. more than one tile per block
def test_a_block_that_walks_several_tiles():
    n, r = 8225, 4
    eng, rng, setup = _chain(n, 1300)
    setup(r)
    zin = rng.standard_normal((65, r, 3))
    worst = max(_check_zeros(eng, n, r, w, zin) for w in (1, 65))
    worst = max(worst, _check_general(eng, n, r, rng, [1, 65]))
    print("chain %d (two tiles per block): largest err / bound %.3g" % (n, worst))
    assert worst < 1.0
