"""GPU (-m gpu): the SPLOCS refinement of csrc/asb_splocs.hip one phase at a time -- the Gram products, the weight sweep in both
kernels, the centres, the fused and the unfused ADMM loop, the host and the device-trace objective, Lambda built on the device --
each against tests/splocs_model.py run in numpy.longdouble on what the device holds.

Every case: upload a small random X, deflate_begin(K, local support), splocs_begin, install a chosen state (asb_test_splocs_install),
run one phase, compare everything the phase wrote (splocs_results, asb_test_splocs_state, the caller's P / M tensors).

Tolerances.  For every compared quantity the float64 model's deviation from the longdouble model on the same inputs is measured
in the test (relative Frobenius norm; largest entry of the difference over the largest entry); the device may deviate from the
longdouble model by MARGIN = 100 times that, and by no less than FLOOR = 50 eps.  The margin covers another order of summation
(4-deep MFMA chunks, 64-lane trees, block partials) and the Gauss-Jordan inverse where the model has a Cholesky one; one wrong or
dropped term is >= 1 / max(F, K, 3 N) ~ 1e-4.  No bound may exceed CEIL = 1e-10 (asserted: rho and the scale of W keep
cond(G + rho I) <= (|W|^2 + rho) / rho small).  Centres, exact zeros and the bit-for-bit equalities have no tolerance.

Largest deviation of the device from the longdouble model observed on an MI355X, per phase (relative Frobenius norm / largest
entry), next to the smallest bound any case of the phase had:

    phase       quantity      observed fro   observed max   smallest bound
    (not measured on a device yet: `pytest -m gpu -s` on this module prints the table, see _report.  For scale, the float64
    model itself deviates from the longdouble one by at most 4.2e-15 / 8.7e-15 (U after four ADMM iterations), 2.1e-15 / 4.6e-15
    (W after a sweep) and below 1.1e-15 in everything else; the smallest bound of every quantity is the floor, 1.1e-14.)
"""
import numpy as np
import pytest

import splocs_model as sm
from oracle import asb_oracle as orc

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
MARGIN, FLOOR, CEIL = 100.0, 50 * EPS, 1e-10
LD = np.longdouble
RHO = 10.0

GRAM_K = (1, 16, 31, 32, 33, 34, 64, 65)
GRAM_F = (17, 64, 100)
GRAM_N = (1, 50, 129)
SWEEP_K = (1, 5, 24, 100, 136)
SWEEP_F = (1, 63, 64, 65, 256, 257, 700)
SWEEP_N = 60
ADMM_K_FUSED = (1, 3, 15, 16, 17, 37, 48, 63, 64)
ADMM_K_UNFUSED = (65, 100)
ADMM_N = (1, 15, 16, 17, 50)
ADMM_ITERS = (1, 4)
ADMM_F = 20
DEAD_CASES = (("zero", "first"), ("below", "last"), ("above", "middle"))

_SEEN = {}              # (phase, quantity) -> [largest fro, largest max, smallest bound]


def sweep_nt(K):
    """rows per block of k_bcd_wide (asb_splocs_weights): what fits the LDS, at most 256; below 64 the one-block kernel runs"""
    return min(((150 * 1024 // 8 - 8) // (K + 1)) // 64 * 64, 256)


def gram_big(K):
    """asb_splocs_gram: P on the 128 x 128-tile kernel (asb_gemm_tn_big) or on the one-wave-per-tile kernel (asb_gemm_tn)"""
    return K >= 32 and K % 2 == 0


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _SEEN:
        print("\n    phase       quantity      observed fro   observed max   smallest bound")
        for (phase, name), (fro, mx, bound) in sorted(_SEEN.items()):
            print("    %-11s %-13s %-14.1e %-14.1e %.1e" % (phase, name, fro, mx, bound))


def check(phase, name, got, lo, hi, where):
    """got (device) against hi (longdouble model) within MARGIN times the deviation of lo (float64 model) from hi"""
    got = np.asarray(got)
    assert np.isfinite(got).all(), (phase, name, where, "not finite")
    ref_fro, ref_max = sm.deviation(lo, hi)
    b_fro, b_max = max(FLOOR, MARGIN * ref_fro), max(FLOOR, MARGIN * ref_max)
    assert b_fro <= CEIL and b_max <= CEIL, (phase, name, where, "the reference alone is above the ceiling", ref_fro, ref_max)
    fro, mx = sm.deviation(got, hi)
    print("%s %s %s: device %.2e / %.2e, float64 model %.2e / %.2e, bound %.2e / %.2e" % (phase, name, where, fro, mx, ref_fro,
                                                                                           ref_max, b_fro, b_max))
    seen = _SEEN.setdefault((phase, name), [0.0, 0.0, np.inf])
    seen[0], seen[1], seen[2] = max(seen[0], fro), max(seen[1], mx), min(seen[2], b_fro, b_max)
    assert fro <= b_fro and mx <= b_max, (phase, name, where, fro, b_fro, mx, b_max)


def _begin(X, K, v0=0, n_loc=None):
    from animsnapbases_amd import HipEngine
    e = HipEngine(0)
    e.upload(X, v0, X.shape[1] if n_loc is None else n_loc)
    e.deflate_begin(K, True)
    e.splocs_begin()
    return e


def _buffers(F, K):
    import torch
    return (torch.full((F * K,), float("nan"), dtype=torch.float64, device="cuda"),
            torch.full((K * K,), float("nan"), dtype=torch.float64, device="cuda"))


def _gram_to(e, P, M, want_norm=False):
    import torch
    torch.cuda.synchronize()
    nx = e.splocs_gram(P.data_ptr(), M.data_ptr(), want_norm)
    e.sync()
    F, K = e.F, e.K
    return P.cpu().numpy().reshape(F, K), M.cpu().numpy().reshape(K, K), nx


def _weights(e, P, M):
    import torch
    torch.cuda.synchronize()
    return e.splocs_weights(P.data_ptr(), M.data_ptr())


# ---------------------------------------------------------------------------------------------------------------- a. Gram
@pytest.mark.parametrize("K", GRAM_K)
def test_gram(K):
    rng = np.random.default_rng(100 + K)
    for F in GRAM_F:
        for n in GRAM_N:
            X = rng.normal(size=(F, n, 3))
            C = rng.normal(size=(K, n, 3))
            e = _begin(X, K)
            try:
                e.test_splocs_install(C=C)
                P, M, nx = _gram_to(e, *_buffers(F, K), want_norm=True)
            finally:
                e.close()
            lo, hi = sm.gram(X, C, np.float64), sm.gram(X, C, LD)
            where = "K=%d F=%d n=%d" % (K, F, n)
            check("gram", "P", P, lo[0], hi[0], where)
            check("gram", "M", M, lo[1], hi[1], where)
            check("gram", "normX2", nx, lo[2], hi[2], where)


# ---------------------------------------------------------------------------------------------------------------- b. sweep
def _sweep_both(monkeypatch, X, C, W0, neg_col, where):
    """one sweep on either kernel from the same state; returns the device's (W, G, P, M) after asserting both against the model
    and against each other bit for bit"""
    F, K = W0.shape
    outs = []
    for wide in ("1", "0"):
        monkeypatch.setenv("ASB_BCD_WIDE", wide)
        e = _begin(X, K)
        try:
            e.test_splocs_install(C=C, W=W0)
            Pt, Mt = _buffers(F, K)
            P, M, _ = _gram_to(e, Pt, Mt)
            if neg_col is not None:         # the caller's (all-reduced) P: a column whose optimum is <= 0 in every frame
                Pt.view(F, K)[:, neg_col] = -(2.0 * np.abs(M).sum() + 1.0)     # < W M[:, k] - M[k, k] W[:, k] whatever W holds
                P = Pt.cpu().numpy().reshape(F, K)
            _weights(e, Pt, Mt)
            W = e.splocs_results()[1]
            G = e.test_splocs_state()["G"]
        finally:
            e.close()
        outs.append((W, G, P, M))
    (W, G, P, M), (W1, G1, P1, M1) = outs
    assert np.array_equal(P, P1) and np.array_equal(M, M1), where
    assert np.array_equal(W, W1), (where, "the two sweep kernels differ")
    assert np.array_equal(G, G1), where
    lo, hi = sm.weights(W0, P, M, np.float64), sm.weights(W0, P, M, LD)
    check("sweep", "W", W, lo, hi, where)
    check("sweep", "G", G, lo.T @ lo, hi.T @ hi, where)
    zero = (hi == 0).all(axis=0)
    assert np.array_equal((W == 0).all(axis=0), zero), (where, "zero columns", np.flatnonzero(zero))
    assert (W.max(axis=0)[~zero] == 1.0).all() and W.min() >= 0.0, where
    return W, G, P, M, zero


def _sweep_state(rng, F, K):
    """X = W_true C + noise and a W off W_true, so that the optimum of (nearly) every column is positive somewhere"""
    C = rng.normal(size=(K, SWEEP_N, 3))
    Wt = rng.uniform(0, 1, size=(F, K))
    X = np.tensordot(Wt, C, (1, 0)) + 0.1 * rng.normal(size=(F, SWEEP_N, 3))
    return X, C, np.clip(Wt + 0.2 * rng.normal(size=(F, K)), 0, 1)


@pytest.mark.parametrize("K", SWEEP_K)
def test_weight_sweep(K, monkeypatch):
    rng = np.random.default_rng(200 + K)
    for F in SWEEP_F:
        X, C, W0 = _sweep_state(rng, F, K)
        neg = K // 2 if K >= 2 else None
        zero = _sweep_both(monkeypatch, X, C, W0, neg, "K=%d F=%d nt=%d" % (K, F, sweep_nt(K)))[4]
        assert zero.tolist() == [k == neg for k in range(K)] or F < 63      # (one or a few frames: some optima are <= 0 by chance)
        assert neg is None or zero[neg]


@pytest.mark.parametrize("kind,pos", DEAD_CASES)
@pytest.mark.parametrize("K", (5, 136))
def test_weight_sweep_dead_components(K, kind, pos, monkeypatch):
    """M[k, k] <= 1e-8 zeroes the column: a component that is exactly zero, one a factor 10 below the threshold, one a factor 10
    above it (which stays live)"""
    rng = np.random.default_rng(300 + K)
    F = 257
    X, C, W0 = _sweep_state(rng, F, K)
    k = {"first": 0, "last": K - 1, "middle": K // 2}[pos]
    C[k] *= {"zero": 0.0, "below": np.sqrt(1e-9 / (C[k] ** 2).sum()), "above": np.sqrt(1e-7 / (C[k] ** 2).sum())}[kind]
    W, G, P, M, zero = _sweep_both(monkeypatch, X, C, W0, None, "K=%d %s %s" % (K, kind, pos))
    assert {"zero": M[k, k] == 0.0, "below": 5e-10 < M[k, k] < 2e-9, "above": 5e-8 < M[k, k] < 2e-7}[kind]
    assert zero.tolist() == [j == k and kind != "above" for j in range(K)]       # (F = 257: no live column is <= 0 throughout)


# ---------------------------------------------------------------------------------------------------------------- c. centres
def _centres(X, C, v0=0, n_loc=None):
    """(centres, values) of the shard's weight phase on its own Gram products"""
    K = C.shape[0]
    n_loc = X.shape[1] if n_loc is None else n_loc
    e = _begin(X, K, v0, n_loc)
    try:
        e.test_splocs_install(C=C[:, v0:v0 + n_loc], W=np.full((X.shape[0], K), 0.5))
        e.splocs_gram()
        return e.splocs_weights()
    finally:
        e.close()


def test_centres_random():
    rng = np.random.default_rng(7)
    K, n = 9, 300
    X = rng.normal(size=(8, n, 3))
    C = rng.normal(size=(K, n, 3))
    en = np.sort((C.astype(LD) ** 2).sum(axis=2), axis=1)
    assert ((en[:, -1] - en[:, -2]) > 1e-6 * en[:, -1]).all(), "precondition: the largest two |C_k[v]|^2 are well apart"
    idx, val = _centres(X, C)
    ref_i, ref_v = sm.centres(C, 0, LD)
    assert idx.tolist() == ref_i.tolist()
    check("centres", "value", val, sm.centres(C, 0, np.float64)[1], ref_v, "random")


def test_centres_exact_ties():
    """integer components: equal |C_k[v]|^2 in one thread's own sequence (v, v + 256), in neighbouring threads, across the
    first level of the block's tree (v, v + 128) and from different coordinates: the lowest index wins"""
    n = 400
    X = np.random.default_rng(8).normal(size=(4, n, 3))
    ties = [(10, 266), (266, 10), (37, 38), (60, 188), (5, 133, 261, 389), (399, 143), (0, 399), (255, 256)]
    shapes = [(3, 4, 0), (0, 0, 5), (5, 0, 0), (0, -4, 3)]
    C = np.zeros((len(ties), n, 3))
    C[:, :, 0] = (np.arange(n) % 3)[None] + 1.0            # background: |.|^2 in {1, 4, 9}, itself full of ties
    C[6] = 0.0                                              # a zero component: every vertex ties, vertex 0 wins
    C[7] = 0.0
    C[7, :, 0] = 2.0                                        # all equal but for the planted pair
    for k, vs in enumerate(ties):
        for j, v in enumerate(vs):
            if k != 6:
                C[k, v] = shapes[(k + j) % 4]              # |.|^2 = 25 in four different ways
    idx, val = _centres(X, C)
    ref_i, ref_v = sm.centres(C, 0, np.float64)
    assert ref_i.tolist() == [10, 10, 37, 60, 5, 143, 0, 255]
    assert idx.tolist() == ref_i.tolist() and np.array_equal(val, ref_v)


def test_centres_and_sweep_on_two_shards():
    """two contexts on one GPU holding [0, n0) and [n0, N): each returns v0 + its winner, merging by (value, lowest index) gives
    the one-rank centres; with P and M summed over the shards both run the same sweep, bit for bit"""
    import torch
    rng = np.random.default_rng(9)
    F, N, n0, K = 70, 300, 130, 7
    X = rng.normal(size=(F, N, 3))
    C = np.rint(rng.normal(size=(K, N, 3)) * 4)
    C[2] = 0
    C[2, [100, 200]] = [[0, 6, 0], [6, 0, 0]]               # tie across the shards: the lower shard's vertex
    C[3] = np.clip(C[3], -2, 2)
    C[3, [120, 140]] = [[1, 1, 1], [9, 0, 0]]               # winner in the upper shard
    C[4, :n0] = 0                                           # nothing in the lower shard
    W0 = rng.uniform(0, 1, size=(F, K))
    shards = [(0, n0), (n0, N - n0)]
    engs, parts = [], []
    try:
        for v0, nl in shards:
            e = _begin(X, K, v0, nl)
            engs.append(e)
            e.test_splocs_install(C=C[:, v0:v0 + nl], W=W0)
            Pt, Mt = _buffers(F, K)
            _gram_to(e, Pt, Mt)
            parts.append((Pt, Mt))
        Ps, Ms = parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]
        res = [_weights(e, Ps, Ms) for e in engs]
        Ws = [e.splocs_results()[1] for e in engs]
    finally:
        for e in engs:
            e.close()
    assert np.array_equal(Ws[0], Ws[1])
    P, M = Ps.cpu().numpy().reshape(F, K), Ms.cpu().numpy().reshape(K, K)
    check("sweep", "W", Ws[0], sm.weights(W0, P, M, np.float64), sm.weights(W0, P, M, LD), "two shards")
    Pm = sm.gram(X, C, LD)
    check("gram", "P", P, sm.gram(X, C, np.float64)[0], Pm[0], "two shards summed")
    check("gram", "M", M, sm.gram(X, C, np.float64)[1], Pm[1], "two shards summed")
    for (v0, nl), (idx, val) in zip(shards, res):
        ref_i, ref_v = sm.centres(C[:, v0:v0 + nl], v0)
        assert idx.tolist() == ref_i.tolist() and np.array_equal(val, ref_v)       # integers: exact
    (i0, x0), (i1, x1) = res
    merged = np.where((x1 > x0) | ((x1 == x0) & (i1 < i0)), i1, i0)
    one_i, one_v = _centres(X, C)
    assert merged.tolist() == one_i.tolist() == sm.centres(C)[0].tolist()
    assert merged[2] == 100 and merged[3] == 140 and merged[4] >= n0
    assert np.array_equal(np.maximum(x0, x1), one_v)


# ---------------------------------------------------------------------------------------------------------------- d. ADMM
def _admm_state(rng, K, n):
    """X, C, U, Lambda with: zeros in Lambda (inside dmin), moderate values, the last component (K >= 2) with Lambda so large
    that all of Z_k becomes 0, and (n >= 2) a last vertex where X, C and U are zero, so that x = C + U = 0 there in every
    iteration, under Lambda > 0 and, in component 0, Lambda = 0"""
    X = rng.normal(size=(ADMM_F, n, 3))
    C = rng.normal(size=(K, n, 3))
    U = 0.3 * rng.normal(size=(K, n, 3))
    Lam = rng.uniform(0, 8, size=(K, n)) * (rng.random((K, n)) > 0.3)
    if n >= 2:
        X[:, -1], C[:, -1], U[:, -1] = 0, 0, 0
        Lam[:, -1] = 1.5
        Lam[0, -1] = 0
    huge = K - 1 if K >= 2 else None
    if huge is not None:
        Lam[huge] = 1e7
    return X, C, U, Lam, huge


def _admm_engine(X, K, C, W0):
    """a context whose W and G = W^T W come from one sweep (G is written by the weight phase alone); returns it with that W"""
    e = _begin(X, K)
    e.test_splocs_install(C=C, W=W0)
    e.splocs_gram()
    e.splocs_weights()
    return e, e.splocs_results()[1]


def _check_admm(e, X, W, C, U, Lam, n_iter, huge, where):
    e.test_splocs_install(C=C, U=U)
    e.splocs_admm(Lam, RHO, n_iter)
    Cd = e.splocs_results()[0]
    st = e.test_splocs_state()
    lo, hi = sm.admm(X, W, C, U, Lam, RHO, n_iter, np.float64), sm.admm(X, W, C, U, Lam, RHO, n_iter, LD)
    assert np.array_equal(st["Lambda"], Lam)
    check("admm", "C", Cd, lo["C"], hi["C"], where)
    check("admm", "U", st["U"], lo["U"], hi["U"], where)
    check("admm", "Ginv", st["Ginv"], lo["Ginv"], hi["Ginv"], where)
    check("admm", "c", st["c"].reshape(C.shape), lo["c"].reshape(C.shape), hi["c"].reshape(C.shape), where)
    if huge is not None:
        assert (hi["C"][huge] == 0).all() and (Cd[huge] == 0).all(), (where, "the component under a huge Lambda is not exactly 0")
    if C.shape[1] >= 2:
        assert (Cd[:, -1] == 0).all() and (st["U"][:, -1] == 0).all(), (where, "x = 0 must give z = 0")
    return Cd, st


@pytest.mark.parametrize("K", ADMM_K_FUSED + ADMM_K_UNFUSED)
def test_admm(K):
    rng = np.random.default_rng(400 + K)
    for n in ADMM_N:
        X, C, U, Lam, huge = _admm_state(rng, K, n)
        e, W = _admm_engine(X, K, C, rng.uniform(0, 1, size=(ADMM_F, K)))
        try:
            for n_iter in ADMM_ITERS:
                _check_admm(e, X, W, C, U, Lam, n_iter, huge, "K=%d n=%d iters=%d" % (K, n, n_iter))
        finally:
            e.close()


@pytest.mark.parametrize("K", (5, 64, 65))
def test_admm_without_iterations_keeps_the_state(K):
    rng = np.random.default_rng(500 + K)
    X, C, U, Lam, _ = _admm_state(rng, K, 17)
    e, W = _admm_engine(X, K, C, rng.uniform(0, 1, size=(ADMM_F, K)))
    try:
        e.test_splocs_install(C=C, U=U)
        e.splocs_admm(Lam, RHO, 0)
        Cd = e.splocs_results()[0]
        st = e.test_splocs_state()
    finally:
        e.close()
    assert np.array_equal(Cd, C) and np.array_equal(st["U"], U) and np.array_equal(st["Lambda"], Lam)
    hi = sm.admm(X, W, C, U, Lam, RHO, 0, LD)
    assert np.array_equal(hi["C"], C) and np.array_equal(hi["U"], U)
    lo = sm.admm(X, W, C, U, Lam, RHO, 0, np.float64)
    check("admm", "Ginv", st["Ginv"], lo["Ginv"], hi["Ginv"], "K=%d iters=0" % K)
    check("admm", "c", st["c"], lo["c"], hi["c"], "K=%d iters=0" % K)


@pytest.mark.parametrize("K", (6, 70))
def test_component_zeroed_by_admm_loses_its_weights(K):
    """two outer iterations the way a run chains them: the ADMM zeroes a component (huge Lambda), the Gram products of the new C
    have M[k, k] = 0, the next sweep zeroes that weight column"""
    rng = np.random.default_rng(600 + K)
    n = 30
    X, C, U, Lam, huge = _admm_state(rng, K, n)
    e, W = _admm_engine(X, K, C, rng.uniform(0, 1, size=(ADMM_F, K)))
    try:
        assert W[:, huge].max() == 1.0
        Cd, st = _check_admm(e, X, W, C, U, Lam, 2, huge, "chain K=%d" % K)
        Pt, Mt = _buffers(ADMM_F, K)
        P, M, _ = _gram_to(e, Pt, Mt)
        _weights(e, Pt, Mt)
        W2 = e.splocs_results()[1]
    finally:
        e.close()
    assert M[huge, huge] == 0.0 and (M[huge] == 0).all() and (P[:, huge] == 0).all()
    hi = sm.weights(W, P, M, LD)
    assert (W2[:, huge] == 0).all() and np.array_equal((W2 == 0).all(axis=0), (hi == 0).all(axis=0))
    assert (hi == 0).all(axis=0).sum() < K // 2
    check("sweep", "W", W2, sm.weights(W, P, M, np.float64), hi, "chain K=%d" % K)


# ---------------------------------------------------------------------------------------------------------------- e. objective
@pytest.mark.parametrize("K", (5, 65))
def test_objective_host_and_device_trace(K):
    rng = np.random.default_rng(700 + K)
    n = 40
    X, C, U, Lam, huge = _admm_state(rng, K, n)
    e, W = _admm_engine(X, K, C, rng.uniform(0, 1, size=(ADMM_F, K)))
    try:
        e.test_splocs_install(C=C, U=U)
        e.splocs_admm(Lam, RHO, 2)
        Pt, Mt = _buffers(ADMM_F, K)
        P, M, _ = _gram_to(e, Pt, Mt)
        host = e.splocs_objective(Pt.data_ptr(), Mt.data_ptr())
        e.splocs_trace_begin(3)
        e.splocs_objective_dev(1, Pt.data_ptr(), Mt.data_ptr())
        tr = e.splocs_trace(3)
        again = e.splocs_objective()            # the context's own copy of P and M
        Cd = e.splocs_results()[0]
        G = e.test_splocs_state()["G"]
    finally:
        e.close()
    assert tr[1].tolist() == list(host) == list(again), "the host and the device-trace objective run the same kernels"
    assert (tr[[0, 2]] == 0).all(), "rows of the trace that no iteration wrote"
    lo, hi = sm.objective(W, G, P, M, Lam, Cd, np.float64), sm.objective(W, G, P, M, Lam, Cd, LD)
    for name, g, a, b in zip(("<W,P>", "<G,M>", "sparsity"), host, lo, hi):
        check("objective", name, g, a, b, "K=%d" % K)


# ---------------------------------------------------------------------------------------------------------------- f. Lambda
@pytest.mark.parametrize("K,v0", [(5, 0), (65, 0), (5, 30)], ids=["argument", "pointer table", "argument, shard"])
def test_lambda_from_cached_fields(K, v0):
    """asb_splocs_admm_fields: the support maps from the distance fields cached on the device, K <= 64 with the field addresses as
    a kernel argument, above through a pointer table, and on a shard [v0, N) (phi + v0)"""
    from animsnapbases_amd.geodesic import GeodesicDistanceComputation
    V, T = orc.synth_mesh(8, 10)
    N = V.shape[0]
    n_loc = N - v0
    lam, dmin, dmax = 2.0, 0.1, 0.4
    rng = np.random.default_rng(800 + K + v0)
    X = rng.normal(size=(ADMM_F, N, 3))
    C = rng.normal(size=(K, n_loc, 3))
    U = 0.3 * rng.normal(size=(K, n_loc, 3))
    # sorted and distinct, so that cache_add and solve_many take the same batches; on a shard some below v0, most inside
    low = rng.permutation(v0)[:K // 2] if v0 else np.zeros(0, dtype=np.int64)
    sources = np.sort(np.concatenate([low, v0 + rng.permutation(n_loc)[:K - low.size]]))
    e = _begin(X, K, v0, n_loc)
    try:
        e.test_splocs_install(C=C, W=rng.uniform(0, 1, size=(ADMM_F, K)))
        e.splocs_gram()
        e.splocs_weights()
        W = e.splocs_results()[1]
        geo = GeodesicDistanceComputation(V, T, engine=e, backend="dense")
        phi = geo.solve_many(sources)
        slots = e.geodesic_cache_add(sources)
        e.test_splocs_install(C=C, U=U)
        e.splocs_admm_fields(slots, lam, dmin, dmax, RHO, 1)
        Cd = e.splocs_results()[0]
        st = e.test_splocs_state()
    finally:
        e.close()
    assert phi.shape == (K, N) and (phi[np.arange(K), sources] < dmin).all() and phi.max() > dmax
    lo, hi = (sm.lambda_from_fields(phi[:, v0:], lam, dmin, dmax, t) for t in (np.float64, LD))
    assert (hi == 0).any() and (hi == lam).any() and ((hi > 0) & (hi < lam)).any()
    where = "K=%d v0=%d" % (K, v0)
    check("lambda", "Lambda", st["Lambda"], lo, hi, where)
    assert np.array_equal(st["Lambda"] == 0, hi == 0) and np.array_equal(st["Lambda"] == lam, hi == lam)
    Xl = X[:, v0:]
    a_lo, a_hi = sm.admm(Xl, W, C, U, st["Lambda"], RHO, 1, np.float64), sm.admm(Xl, W, C, U, st["Lambda"], RHO, 1, LD)
    check("lambda", "C", Cd, a_lo["C"], a_hi["C"], where)
    check("lambda", "U", st["U"], a_lo["U"], a_hi["U"], where)


# ---------------------------------------------------------------------------------------------------------------- coverage
def test_cases_cover_the_edges():
    """The case tables themselves: every K, F and n_loc class and both sides of every switch at least once."""
    fused, unfused = set(ADMM_K_FUSED), set(ADMM_K_UNFUSED)
    assert max(fused) == 64 and min(unfused) == 65                                   # the 64 -> 65 switch to the unfused loop
    assert any(k % 4 for k in fused) and 1 in fused                                  # a partly zero last MFMA k-chunk; K = 1
    assert any(32 < k < 64 and k % 16 for k in fused)                                # waves 2 and 3 with partly live rows
    assert {n for n in ADMM_N if n < 16} and 16 in ADMM_N and any(n > 16 and n % 16 for n in ADMM_N)
    assert set(ADMM_ITERS) == {1, 4}
    nts = {sweep_nt(K) for K in SWEEP_K}
    assert 256 in nts and 128 in nts                                                 # an nt = 128 sweep next to the full blocks
    for K in SWEEP_K:
        nt = sweep_nt(K)
        assert any(F % nt == 0 for F in SWEEP_F) and any(F % nt and F > nt for F in SWEEP_F), K   # an exactly full and a ragged last block
    assert any(F < 64 for F in SWEEP_F) and 1 in SWEEP_F and 700 in SWEEP_F
    assert any(gram_big(K) for K in GRAM_K) and any(not gram_big(K) for K in GRAM_K)  # both Gram branches
    assert any(not gram_big(K) and K > 32 for K in GRAM_K) and any(not gram_big(K) and K < 32 and not K % 2 for K in GRAM_K)
    assert {32, 64} <= set(GRAM_K) and any(F % 16 for F in GRAM_F) and any(not F % 16 for F in GRAM_F)
    assert 1 in GRAM_N and any(n % 16 for n in GRAM_N)
    assert {c[0] for c in DEAD_CASES} == {"zero", "below", "above"} and {"first", "last"} <= {c[1] for c in DEAD_CASES}
