"""GPU (-m gpu): the constraint-basis chain of config 5 one entry point at a time -- asb_orth_gram, one CholeskyQR pass per slice
and joint, CholeskyQR2, the QR refusals, asb_pod_basis / asb_pod_basis_dev, asb_pod_project, asb_pod_rotate, asb_pod_power,
asb_pod_deflate_begin / _end over two levels, asb_snapshots_affine, asb_components_post, asb_components_truncate -- each against
tests/pod_model.py run in numpy.longdouble on what the device holds.

Every case uploads small random inputs, runs one entry point, reads back everything it wrote and compares with the model fed
the device's own inputs: where a phase consumes a device-made Gram matrix, V, lambda, B or S, that is read back and handed to
the model, so that each test judges one phase.  The branch a case takes is named by the predicates below (orth_syrk,
combine_rows_ok, basis_gemm, chol_one_block, chol_lds_optin), which mirror the conditions in the C code;
test_cases_cover_the_edges asserts that the case tables reach both sides of each.

Tolerances.  For every compared quantity the float64 model's deviation from the longdouble model on the same inputs is measured
in the test (relative Frobenius norm; largest entry of the difference over the largest entry); the device may deviate from the
longdouble model by MARGIN = 100 times that, and by no less than FLOOR = 50 eps.  The margin covers another order of summation
(4-deep MFMA chunks, split-K slabs, 64-lane trees) and the blocked Cholesky where the model has an unblocked one.  No bound may
exceed CEIL = 1e-10 (asserted: a condition on the inputs).  CholeskyQR2 is judged by its orthogonality defect, which may be
MARGIN times the float64 model's (and no less than FLOOR).  The element-wise kernels (affine, components_post) get 2 eps per
entry relative to the sum of the magnitudes of the model's terms: three roundings of half an eps each, fewer with an FMA.
Bit-for-bit assertions have no tolerance: a caller's buffer against the context, the 4 G pass, refusals leaving the state
unchanged, the restoration of X, a second cycle against a fresh engine, truncation.

What asb_pod_basis / asb_pod_basis_dev return for an eigenvalue <= 0 (test_basis_nonpositive_eigenvalue): sigma = sqrt(max(
lambda, 0)) = 0 and the row is divided by it, so exactly those basis rows hold inf / NaN and nothing else does; the callers in
constraints.py never ask for such a row (they cut K at the resolved part of the spectrum first).

Largest deviation of the device from the longdouble model observed on an MI355X, per phase (relative Frobenius norm / largest
entry), next to the smallest bound any case of the phase had:

    phase       quantity      observed fro   observed max   smallest bound
    affine      X / eps       9.6e-01        9.6e-01        2.0e+00
    affine      back / eps    7.8e-01        7.8e-01        2.0e+00
    affine      gram after    4.8e-16        1.8e-15        1.1e-14
    comps_post  C / eps       1.0e+00        1.0e+00        2.0e+00
    orth_gram   G             3.3e-16        7.9e-16        1.1e-14
    pod_basis   dev           7.9e-16        3.0e-15        1.1e-14
    pod_basis   host          8.1e-16        3.0e-15        1.1e-14
    pod_deflate A             8.8e-17        1.8e-16        1.1e-14
    pod_deflate qr after      1.9e-16        3.0e-16        1.1e-14
    pod_gram    G             3.0e-16        6.8e-16        1.1e-14
    pod_power   basis         4.0e-16        6.7e-16        1.1e-14
    pod_project B             4.1e-16        7.9e-16        1.1e-14
    pod_rotate  S             1.6e-14        2.1e-14        1.1e-14
    pod_rotate  basis         3.1e-14        5.8e-14        1.1e-14
    pod_rotate  rows          2.5e-14        2.9e-14        1.1e-14
    pod_rotate  signs         2.8e-15        2.8e-15        1.1e-14
    qr2         defect        5.5e-16        1.4e-15        2.9e-14
    qr_apply    basis         5.7e-16        1.2e-15        1.1e-14
    qr_joint    basis         4.1e-16        8.3e-16        1.1e-14
    qr_joint    routes        2.8e-16        6.1e-16        2.1e-14

("/ eps" rows: the largest entry-wise error in units of eps times the terms, bound 2.  The largest figures of pod_rotate are
those of K = 128, where the float64 Jacobi of the model is itself 3.6e-14 / 8.7e-14 away from the longdouble one and the bound
is 3.6e-12 / 8.7e-12; the smallest bound in its rows is the floor, at K = 1.)  The margin of 100 was enough in every phase.

No defect was found.  What the phases rule out was tried on scratch builds with one arithmetic change each (every access still
in bounds), each run once against this module: k_sum3 without the third slice -- 22 tests fail (every joint pass, CholeskyQR2
joint, the QR after the deflation levels); the per-slice pass with slice 0's factor for all three -- 15 (every per-slice pass);
k_chol_tinv's trailing update without the diagonal -- 28 (every K from 2 to 128 on the one-block path); k_power_v and k_gather_b
without the sorted-to-stored map -- test_pod_power at K = 64 and 128, all of test_pod_deflate_levels; rowscale[r / 4] in
k_affine_rows -- all of test_snapshots_affine and the grid-stride case; K in place of eig_k as the leading dimension of the
vectors in asb_pod_basis_dev -- test_pod_basis[130] (the only F with room for K + 2 vectors on the GEMM route); mean added before
the division in k_comps_post -- all of test_components_post.
"""
import numpy as np
import pytest

import pod_model as pm

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
MARGIN, FLOOR, CEIL = 100.0, 50 * EPS, 1e-10
LD = np.longdouble

GRAM_K = (1, 2, 63, 64, 65, 66)
GRAM_N = (1, 5, 129)
QR_K = (1, 2, 63, 64, 65, 78, 79, 80, 127, 128, 129, 130)
QR2_K = (64, 128, 130)
REFUSE_K = (5, 100, 130)
BASIS_F = (3, 63, 64, 65, 130)
BASIS_K = (1, 16, 17, 63, 64, 65, 66)
BASIS_N = (33, 34)


def BASIS_KV(K):
    """the k of asb_sym_eig_topk = the leading dimension of its vectors: K, K + 1 (odd or even next to K) and K + 2 (the parity
    of K with a leading dimension that is not K, which the GEMM route of asb_pod_basis_dev needs)"""
    return (K, K + 1, K + 2)


PROJ_K = (1, 17, 63, 64, 65, 66)
PROJ_F = (3, 64, 65)
PROJ_N = (1, 33, 34)
ROT_K = (1, 2, 5, 64, 65, 128)
POWER_K = (2, 64, 128)
DEFLATE_SHAPES = ((8, 6, 6, 4), (70, 130, 64, 66))       # (F, n_loc, K of level 1, K of level 2)
AFFINE_F = (1, 63, 64, 65)
AFFINE_N = (1, 2, 100)
ROWS_PER_BLOCK = 4          # k_affine_rows: one wave per row, four waves per block
POST_PER_BLOCK = 256        # k_comps_post: one entry per thread

_SEEN = {}              # (phase, quantity) -> [largest fro, largest max, smallest bound]


# ---------------------------------------------------------------------------------------------------------------- branches
def orth_syrk(K):
    """asb_orth_gram: asb_syrk_tn on the strided slice rows, else asb_gemm_tn; asb_pod_project: asb_gemm_tn_big, else
    asb_gemm_tn"""
    return K >= 64 and K % 2 == 0


def combine_rows_ok(K, n_loc):
    """asb_combine_rows_ok: the joint pass / the rotation as one (K x K)(K x 3n) asb_gemm_nn, else three strided asb_gemm_tn_s"""
    return K >= 64 and K % 2 == 0 and (3 * n_loc) % 2 == 0


def basis_gemm(K, n_loc, F, eig_k):
    """asb_pod_basis_dev: asb_gemm_nn + k_transpose_div, else 16 columns per pass of the projection kernel"""
    return K >= 64 and not (K % 2 or (3 * n_loc) % 2 or F % 2 or eig_k % 2)


def chol_one_block(K):
    """qr_apply: k_chol_tinv in one block's LDS, else the blocked asb_chol_tinv_dev"""
    return K <= 128


def chol_lds_optin(K):
    """k_chol_tinv's K^2 doubles of LDS are above the 48 KB a kernel gets without hipFuncSetAttribute"""
    return chol_one_block(K) and K * K * 8 > 48 * 1024


def grid_cap():
    """ctx->nblk_cap (asb_snapshots.hip): eight blocks per compute unit, the grid cap of the streaming kernels"""
    import torch
    return 8 * torch.cuda.get_device_properties(0).multi_processor_count


# ---------------------------------------------------------------------------------------------------------------- plumbing
@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _SEEN:
        print("\n    phase       quantity      observed fro   observed max   smallest bound")
        for (phase, name), (fro, mx, bound) in sorted(_SEEN.items()):
            print("    %-11s %-13s %-14.1e %-14.1e %.1e" % (phase, name, fro, mx, bound))


def check(phase, name, got, lo, hi, where, ref=None):
    """got (device) against hi (longdouble model) within MARGIN times the deviation of lo (float64 model) from hi; ``ref``: that
    deviation measured on another quantity of the same computation, where got has no model of its own.  Returns the deviations."""
    got = np.asarray(got)
    assert np.isfinite(got).all(), (phase, name, where, "not finite")
    ref_fro, ref_max = pm.deviation(lo, hi) if ref is None else ref
    b_fro, b_max = max(FLOOR, MARGIN * ref_fro), max(FLOOR, MARGIN * ref_max)
    assert b_fro <= CEIL and b_max <= CEIL, (phase, name, where, "the reference alone is above the ceiling", ref_fro, ref_max)
    fro, mx = pm.deviation(got, hi)
    print("%s %s %s: device %.2e / %.2e, float64 model %.2e / %.2e, bound %.2e / %.2e" % (phase, name, where, fro, mx, ref_fro,
                                                                                           ref_max, b_fro, b_max))
    seen = _SEEN.setdefault((phase, name), [0.0, 0.0, np.inf])
    seen[0], seen[1], seen[2] = max(seen[0], fro), max(seen[1], mx), min(seen[2], b_fro, b_max)
    assert fro <= b_fro and mx <= b_max, (phase, name, where, fro, b_fro, mx, b_max)
    return ref_fro, ref_max


def _engine(X):
    from animsnapbases_amd import HipEngine
    e = HipEngine(0)
    e.upload(X, 0, X.shape[1])
    return e


def _basis_engine(C, F=3):
    """a context holding the basis C (K, n, 3) and zero snapshots of F frames (a basis needs a tensor to belong to)"""
    e = _engine(np.zeros((F, C.shape[1], 3)))
    e.components_upload(C)
    return e


def _tensor(a=None, size=None):
    """a caller-owned device tensor: a copy of ``a``, or ``size`` NaNs; ready before the engine's stream reads it"""
    import torch
    t = (torch.full((size,), float("nan"), dtype=torch.float64, device="cuda") if a is None
         else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda").reshape(-1))
    torch.cuda.synchronize()
    return t


def _host(e, t, shape):
    e.sync()
    return t.cpu().numpy().reshape(shape).copy()


def _orthonormal(rng, rows, cols):
    """(rows, cols) with orthonormal columns"""
    return np.linalg.qr(rng.normal(size=(rows, cols)))[0]


def _prescribed_b(rng, K, F, s):
    """U diag(s) V^T (K, F) with U (K, K) orthogonal and V (F, K) orthonormal columns"""
    return (_orthonormal(rng, K, K) * s[None]) @ _orthonormal(rng, F, K).T


def _sorted_rows(B_rot, S):
    """the device's rotated rows in S's order: the stored-to-sorted map is recovered from the row norms, which are distinct"""
    norms = np.sqrt((B_rot.astype(LD) ** 2).sum(axis=1))
    order = np.argsort(-norms, kind="stable")
    assert np.allclose(norms[order].astype(np.float64), S, rtol=1e-9, atol=0), "row norms of the rotated B are not S"
    assert len(S) < 2 or (S[:-1] > S[1:]).all(), "precondition: distinct singular values"
    return B_rot[order]


# ---------------------------------------------------------------------------------------------------------------- a. orth_gram
@pytest.mark.parametrize("K", GRAM_K)
def test_orth_gram(K):
    rng = np.random.default_rng(1000 + K)
    for n in GRAM_N:
        C = rng.normal(size=(K, n, 3))
        e = _basis_engine(C)
        try:
            e.orth_gram()
            G = e.orth_gram_get()
            Gt = _tensor(size=3 * K * K)
            e.orth_gram(Gt.data_ptr())
            G2 = _host(e, Gt, (3, K, K))
            assert np.array_equal(e.orth_gram_get(), G), "a caller's buffer must leave the context's Gram matrices alone"
        finally:
            e.close()
        where = "K=%d n=%d %s" % (K, n, "syrk" if orth_syrk(K) else "gemm_tn")
        assert np.array_equal(G, G2), (where, "context and caller's tensor differ")
        check("orth_gram", "G", G, pm.slice_grams(C, np.float64), pm.slice_grams(C, LD), where)
        if orth_syrk(K):
            assert np.array_equal(G, G.transpose(0, 2, 1)), (where, "the SYRK result is not exactly symmetric")


# ---------------------------------------------------------------------------------------------------------------- b. one QR pass
def _qr_pass(C, joint, G_scale=None):
    """(G read back, basis after one pass); G_scale: the pass reads G_scale * G from a caller's tensor, the context keeps G"""
    e = _basis_engine(C)
    try:
        e.orth_gram()
        G = e.orth_gram_get()
        Gt = None if G_scale is None else _tensor(G_scale * G)
        (e.qr_apply_joint if joint else e.qr_apply)(None if Gt is None else Gt.data_ptr())
        return G, e.results_comps()
    finally:
        e.close()


def _qr_where(K, n, joint):
    chol = "one block%s" % (" > 48 KB" if chol_lds_optin(K) else "") if chol_one_block(K) else "blocked"
    return "K=%d n=%d %s, %s" % (K, n, chol, ("combine_rows" if combine_rows_ok(K, n) else "strided") if joint else "per slice")


@pytest.mark.parametrize("joint", (False, True), ids=("slices", "joint"))
@pytest.mark.parametrize("K", QR_K)
def test_qr_pass(K, joint):
    rng = np.random.default_rng(2000 + K)
    phase = "qr_joint" if joint else "qr_apply"
    for n in (2 * K + 1, 2 * K + 2) + ((K,) if joint and K % 2 == 0 else ()):
        C = rng.normal(size=(K, n, 3))
        where = _qr_where(K, n, joint)
        G, Q = _qr_pass(C, joint)
        check(phase, "basis", Q, pm.chol_qr(C, G, joint, np.float64), pm.chol_qr(C, G, joint, LD), where)
        # lower triangular in the old basis: component j is a combination of the components <= j
        if K >= 2:
            C2 = C.copy()
            C2[K - 1] = rng.normal(size=(n, 3))
            Q2 = _qr_pass(C2, joint)[1]
            assert np.array_equal(Q2[:K - 1], Q[:K - 1]), (where, "component K - 1 leaks into the earlier ones")
            assert not np.array_equal(Q2[K - 1], Q[K - 1])
        # the caller's Gram matrices are the ones used: 4 G gives L -> 2 L, T -> T / 2 exactly
        Gh, Qh = _qr_pass(C, joint, 4.0)
        assert np.array_equal(Gh, G) and np.array_equal(Qh, 0.5 * Q), (where, "4 G in the caller's tensor must halve the basis")


@pytest.mark.parametrize("K", (64, 128, 130))
def test_qr_joint_routes_agree(K):
    """the same basis with 3 n odd (three strided products) and, padded by one zero vertex, 3 n even (one product)"""
    rng = np.random.default_rng(2500 + K)
    n = 2 * K + 1
    C = rng.normal(size=(K, n, 3))
    Cp = np.concatenate([C, np.zeros((K, 1, 3))], axis=1)
    assert not combine_rows_ok(K, n) and combine_rows_ok(K, n + 1)
    G, Q = _qr_pass(C, True)
    Gp, Qp = _qr_pass(Cp, True)
    lo, hi = pm.chol_qr(C, G, True, np.float64), pm.chol_qr(C, G, True, LD)
    check("qr_joint", "routes", Qp[:, :n], lo, hi, "K=%d padded against unpadded" % K)
    check("qr_joint", "routes", Q, lo, hi, "K=%d unpadded" % K)
    assert (Qp[:, n] == 0).all(), "the zero vertex must stay zero"


# ---------------------------------------------------------------------------------------------------------------- c. CholeskyQR2
@pytest.mark.parametrize("joint", (False, True), ids=("slices", "joint"))
@pytest.mark.parametrize("K", QR2_K)
def test_cholesky_qr2(K, joint):
    rng = np.random.default_rng(3000 + K)
    for n in (2 * K + 1, 2 * K + 2):
        C = rng.normal(size=(K, n, 3))
        e = _basis_engine(C)
        try:
            for _ in range(2):
                e.orth_gram()
                (e.qr_apply_joint if joint else e.qr_apply)()
            Q = e.results_comps()
        finally:
            e.close()
        M = C
        for _ in range(2):
            M = pm.chol_qr(M, pm.slice_grams(M, np.float64), joint, np.float64)
        (fro, mx), (r_fro, r_max) = pm.orth_defect(Q, joint), pm.orth_defect(M, joint)
        b_fro, b_max = max(FLOOR, MARGIN * r_fro), max(FLOOR, MARGIN * r_max)
        where = _qr_where(K, n, joint)
        print("qr2 defect %s: device %.2e / %.2e, float64 model %.2e / %.2e, bound %.2e / %.2e" % (where, fro, mx, r_fro, r_max,
                                                                                                    b_fro, b_max))
        seen = _SEEN.setdefault(("qr2", "defect"), [0.0, 0.0, np.inf])
        seen[0], seen[1], seen[2] = max(seen[0], fro), max(seen[1], mx), min(seen[2], b_fro, b_max)
        assert np.isfinite(Q).all() and b_fro <= CEIL and b_max <= CEIL
        assert fro <= b_fro and mx <= b_max, (where, fro, b_fro, mx, b_max)


# ---------------------------------------------------------------------------------------------------------------- d. refusals
@pytest.mark.parametrize("joint", (False, True), ids=("slices", "joint"))
@pytest.mark.parametrize("K", REFUSE_K)
def test_qr_refuses_a_zero_component(K, joint):
    """an all-zero component makes its pivot exactly 0: RuntimeError, the basis untouched, and the next valid call on the same
    engine matches a fresh one bit for bit"""
    rng = np.random.default_rng(4000 + K)
    n = 2 * K + 2
    bad = rng.normal(size=(K, n, 3))
    bad[K // 2] = 0.0
    good = rng.normal(size=(K, n, 3))
    e = _basis_engine(bad)
    try:
        e.orth_gram()
        with pytest.raises(RuntimeError, match="rank deficient"):
            (e.qr_apply_joint if joint else e.qr_apply)()
        assert np.array_equal(e.results_comps(), bad), "a refused pass changed the basis"
        e.components_upload(good)
        e.orth_gram()
        G = e.orth_gram_get()
        (e.qr_apply_joint if joint else e.qr_apply)()
        Q = e.results_comps()
    finally:
        e.close()
    G1, Q1 = _qr_pass(good, joint)
    assert np.array_equal(G, G1) and np.array_equal(Q, Q1), "the pass after a refusal differs from a fresh engine's"
    with pytest.raises(ValueError, match="rank deficient"):
        pm.chol_qr(bad, pm.slice_grams(bad, LD), joint, LD)


# ---------------------------------------------------------------------------------------------------------------- e. pod_basis
def _low_rank_plus_noise(rng, F, n, floor=3e-2):
    """(F, n, 3) whose matrix A (3 n, F) has singular values geometric from 1 down to ``floor``: sigma_K / sigma_0 >= 1e-3"""
    r = min(F, 3 * n)
    A = (_orthonormal(rng, 3 * n, r) * np.geomspace(1.0, floor, r)[None]) @ _orthonormal(rng, F, r).T
    return pm.unrows(A, n)


def _basis_both_routes(e, X, K, Kv, G_dev_ptr=None):
    """(lam, V, basis of pod_basis_dev, basis of pod_basis) from one eigen-solve of Kv vectors"""
    lam, V, _ = e.sym_eig_topk(e.F, Kv, G_dev_ptr, want_vectors=True)
    e.pod_basis_dev(K)
    Cd = e.results_comps()
    e.pod_basis(np.ascontiguousarray(V[:, :K]), np.sqrt(np.maximum(lam[:K], 0.0)))
    return lam, V, Cd, e.results_comps()


@pytest.mark.parametrize("F", BASIS_F)
def test_pod_basis(F):
    rng = np.random.default_rng(5000 + F)
    for n in BASIS_N:
        X = _low_rank_plus_noise(rng, F, n)
        e = _engine(X)
        try:
            G = e.pod_gram()
            A = pm.rows(X, LD)
            check("pod_gram", "G", G, pm.rows(X).T @ pm.rows(X), A.T @ A, "F=%d n=%d" % (F, n))
            for K in BASIS_K:
                for Kv in BASIS_KV(K):
                    if Kv > F:
                        continue
                    e.pod_gram(to_host=False)               # (the eigen-solver works in the context's Gram matrix)
                    lam, V, Cd, Ch = _basis_both_routes(e, X, K, Kv)
                    assert lam[K - 1] > 1e-6 * lam[0] > 0, "precondition: sigma_K / sigma_0 >= 1e-3"
                    lo, hi = pm.basis(X, V, lam, K, np.float64), pm.basis(X, V, lam, K, LD)
                    where = "F=%d n=%d K=%d Kv=%d" % (F, n, K, Kv)
                    check("pod_basis", "dev", Cd, lo, hi, where + (" gemm_nn" if basis_gemm(K, n, F, Kv) else " 16 columns"))
                    check("pod_basis", "host", Ch, lo, hi, where)
        finally:
            e.close()


@pytest.mark.parametrize("F,n,K", [(8, 5, 8), (66, 34, 66)], ids=("16 columns", "gemm_nn"))
def test_basis_nonpositive_eigenvalue(F, n, K):
    """eigenvalues <= 0 (the Gram matrix in a caller's tensor, shifted down past its two smallest eigenvalues): sigma = 0, the
    division is not guarded, and exactly those rows of the basis are inf / NaN; the others equal the model"""
    rng = np.random.default_rng(5500 + F)
    X = _low_rank_plus_noise(rng, F, n, floor=0.1)
    assert basis_gemm(K, n, F, K) == (K >= 64)
    e = _engine(X)
    try:
        G = e.pod_gram()
        w = np.linalg.eigvalsh(G)
        Gt = _tensor(G - 0.5 * (w[1] + w[2]) * np.eye(F))
        lam, V, Cd, Ch = _basis_both_routes(e, X, K, K, Gt.data_ptr())
    finally:
        e.close()
    dead = lam[:K] <= 0
    assert dead.tolist() == [k >= K - 2 for k in range(K)], lam
    hi = pm.basis(X, V, lam, K, LD)
    assert not np.isfinite(hi[dead]).any()
    for name, C in (("dev", Cd), ("host", Ch)):
        assert not np.isfinite(C[dead]).any(), (name, "a row divided by sigma = 0 holds finite values")
        check("pod_basis", name, C[~dead], pm.basis(X, V, lam, K, np.float64)[~dead], hi[~dead], "F=%d lambda <= 0" % F)


# ---------------------------------------------------------------------------------------------------------------- f. pod_project
@pytest.mark.parametrize("K", PROJ_K)
def test_pod_project(K):
    rng = np.random.default_rng(6000 + K)
    for F in PROJ_F:
        for n in PROJ_N:
            X = rng.normal(size=(F, n, 3))
            C = rng.normal(size=(K, n, 3))
            e = _engine(X)
            try:
                e.components_upload(C)
                B = e.pod_project()
                Bt = _tensor(size=K * F)
                Bh = e.pod_project(Bt.data_ptr())
                B2 = _host(e, Bt, (K, F))
            finally:
                e.close()
            where = "K=%d F=%d n=%d %s" % (K, F, n, "gemm_tn_big" if orth_syrk(K) else "gemm_tn")
            assert np.array_equal(B, B2) and np.array_equal(Bh, B2), (where, "context and caller's tensor differ")
            check("pod_project", "B", B, pm.project(C, X, np.float64), pm.project(C, X, LD), where)


# ---------------------------------------------------------------------------------------------------------------- g. pod_rotate
def _rotate(e, B):
    """(S, new basis, the rotated rows as stored, the tensor) of asb_pod_rotate on B in a caller's tensor"""
    Bt = _tensor(B)
    S = e.pod_rotate(Bt.data_ptr())
    return S, e.results_comps(), _host(e, Bt, B.shape), Bt


def _check_rotate(Q, B, small, S, Cn, B_rot, where):
    """the device's (S, basis, rows) against the model's; small: pm.rotate_rows(B) in float64 and in longdouble"""
    lo, hi = pm.rotate(Q, B, np.float64, small[0]), pm.rotate(Q, B, LD, small[1])
    check("pod_rotate", "S", S, lo[0], hi[0], where)
    check("pod_rotate", "basis", pm.align_signs(Cn, hi[3]), pm.align_signs(lo[3], hi[3]), hi[3], where)
    Bs = _sorted_rows(B_rot, S)
    ref = check("pod_rotate", "rows", pm.align_signs(Bs, hi[2]), pm.align_signs(lo[2], hi[2]), hi[2], where)
    # one sign for a basis vector and its row: new_basis[r] = u_r^T Q with Q orthonormal, so (new_basis Q^T) B is row r again
    u = pm.flat(Cn, LD) @ pm.flat(Q, LD).T
    check("pod_rotate", "signs", Bs, None, u @ np.asarray(B, dtype=LD), where, ref=ref)


@pytest.mark.parametrize("K", ROT_K)
def test_pod_rotate(K):
    rng = np.random.default_rng(7000 + K)
    F = K + 6
    B = _prescribed_b(rng, K, F, np.geomspace(1.0, 1e-2, K))
    small = pm.rotate_rows(B, np.float64), pm.rotate_rows(B, LD)         # (B is the same for both n: one small SVD per type)
    for n in (K + 1, K + 2):
        Q = _orthonormal(rng, 3 * n, K).T.reshape(K, n, 3)
        e = _engine(np.zeros((F, n, 3)))
        try:
            e.components_upload(Q)
            S, Cn, B_rot, _ = _rotate(e, B)
        finally:
            e.close()
        _check_rotate(Q, B, small, S, Cn, B_rot, "K=%d n=%d %s" % (K, n, "combine_rows" if combine_rows_ok(K, n) else "strided"))


# ---------------------------------------------------------------------------------------------------------------- h. pod_power
@pytest.mark.parametrize("K", POWER_K)
def test_pod_power(K):
    """directly after a rotation, K, F and 3 n even; then with one exactly zero row in B"""
    rng = np.random.default_rng(8000 + K)
    F, n = K + 6, K + 2
    X = rng.normal(size=(F, n, 3))
    Q = _orthonormal(rng, 3 * n, K).T.reshape(K, n, 3)
    B = _prescribed_b(rng, K, F, np.geomspace(1.0, 1e-2, K))
    Bz = np.insert(_prescribed_b(rng, K - 1, F, np.geomspace(1.0, 1e-2, K - 1)), K // 2, 0.0, axis=0)
    for kind, Bk in (("full", B), ("zero row", Bz)):
        e = _engine(X)
        try:
            e.components_upload(Q)
            S, Cn, B_rot, Bt = _rotate(e, Bk)
            if kind == "full":
                Bs = _sorted_rows(B_rot, S)
            else:
                assert S[-1] == 0.0 and (B_rot[K // 2] == 0).all(), "the zero row must stay exactly zero"
                Bs = np.concatenate([_sorted_rows(np.delete(B_rot, K // 2, axis=0), S[:-1]), np.zeros((1, F))])
            e.pod_power(Bt.data_ptr())
            P = e.results_comps()
            assert np.array_equal(_host(e, Bt, Bk.shape), B_rot), "asb_pod_power must not write B"
        finally:
            e.close()
        check("pod_power", "basis", P, pm.power(X, Bs, S, np.float64), pm.power(X, Bs, S, LD), "K=%d %s" % (K, kind))
        if kind == "zero row":
            assert (P[-1] == 0).all() and (P[:-1] != 0).any(axis=(1, 2)).all(), "sigma = 0 must give an exactly zero basis row"


@pytest.mark.parametrize("K,F,n", [(5, 10, 6), (4, 9, 6), (4, 10, 5)], ids=("K odd", "F odd", "3n odd"))
def test_pod_power_refuses_odd_dimensions(K, F, n):
    rng = np.random.default_rng(8500 + K + F + n)
    X = rng.normal(size=(F, n, 3))
    Q = _orthonormal(rng, 3 * n, K).T.reshape(K, n, 3)
    e = _engine(X)
    try:
        e.components_upload(Q)
        S, Cn, B_rot, Bt = _rotate(e, _prescribed_b(rng, K, F, np.geomspace(1.0, 1e-2, K)))
        with pytest.raises(RuntimeError, match="odd dimension"):
            e.pod_power(Bt.data_ptr())
        assert np.array_equal(e.results_comps(), Cn) and np.array_equal(e.download_snapshots(), X)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- i. levels
def _two_groups(rng, F, n):
    """(F, n, 3) with two well-separated groups of singular values: two around 1, the others around 1e-3"""
    r = min(F, 3 * n)
    s = np.concatenate([[1.0, 0.7], np.geomspace(2e-3, 5e-4, r - 2)])
    return pm.unrows((_orthonormal(rng, 3 * n, r) * s[None]) @ _orthonormal(rng, F, r).T, n)


def _level(e, C, keep, where):
    """one level as production runs it: upload the basis, project, rotate, keep the leading rows and deflate; checks the deflated
    tensor against the model on the device's own operands and returns (kept rows, deflated tensor)"""
    X0 = e.download_snapshots()
    e.components_upload(C)
    K, F = C.shape[0], e.F
    Bt = _tensor(size=K * F)
    e.pod_project(Bt.data_ptr(), to_host=False)
    S = e.pod_rotate(Bt.data_ptr())
    Cn, Bs = e.results_comps(), _sorted_rows(_host(e, Bt, (K, F)), S)
    e.pod_deflate_begin(keep, Bt.data_ptr())
    X1 = e.download_snapshots()
    assert np.array_equal(e.results_comps(), Cn), "asb_pod_deflate_begin must not write the basis"
    check("pod_deflate", "A", X1, pm.deflate(X0, Cn[:keep], Bs[:keep], np.float64), pm.deflate(X0, Cn[:keep], Bs[:keep], LD),
          where)
    return Cn[:keep], X1


def _cycle(e, X, bases, last, where):
    """begin, begin, a third basis, end(last): everything read back on the way"""
    kept1, X1 = _level(e, bases[0], 2, where + " level 1")
    kept2, X2 = _level(e, bases[1], 2, where + " level 2")
    assert not np.array_equal(X1, X2)
    e.components_upload(bases[2])
    e.pod_deflate_end(last, 4 + last)
    grown = e.results_comps()
    assert grown.shape[0] == 4 + last
    assert np.array_equal(grown, np.concatenate([kept1, kept2, bases[2][:last]])), (where, "[kept ; kept ; last] not installed")
    assert np.array_equal(e.download_snapshots(), X), (where, "the snapshots are not restored bit for bit")
    # the replaced basis buffer serves the next QR pass (its capacity bookkeeping)
    e.orth_gram()
    G = e.orth_gram_get()
    e.qr_apply_joint()
    Qg = e.results_comps()
    check("pod_deflate", "qr after", Qg, pm.chol_qr(grown, G, True, np.float64), pm.chol_qr(grown, G, True, LD), where)
    return X1, X2, grown, G, Qg


@pytest.mark.parametrize("last", (0, 2))
@pytest.mark.parametrize("F,n,K1,K2", DEFLATE_SHAPES, ids=("small", "big"))
def test_pod_deflate_levels(F, n, K1, K2, last):
    rng = np.random.default_rng(9000 + F + last)
    X = _two_groups(rng, F, n)
    bases = [_orthonormal(rng, 3 * n, k).T.reshape(k, n, 3) for k in (K1, K2, 4)]
    where = "F=%d n=%d K=%d,%d last=%d" % (F, n, K1, K2, last)
    e = _engine(X)
    try:
        first = _cycle(e, X, bases, last, where)
        again = _cycle(e, X, bases, last, where + " again")
        with pytest.raises(RuntimeError, match="without asb_pod_deflate_begin"):
            e.pod_deflate_end(0, 0)
    finally:
        e.close()
    for a, b in zip(first, again):
        assert np.array_equal(a, b), (where, "a second cycle on the same engine differs from the first on a fresh one")


def _refusal_engine(rng, F, n, K):
    """a context after project + rotate (so that only the argument under test can be refused): (engine, X, basis, B tensor)"""
    X = _two_groups(rng, F, n)
    e = _engine(X)
    e.components_upload(_orthonormal(rng, 3 * n, K).T.reshape(K, n, 3))
    Bt = _tensor(size=K * F)
    e.pod_project(Bt.data_ptr(), to_host=False)
    e.pod_rotate(Bt.data_ptr())
    return e, X, e.results_comps(), Bt


@pytest.mark.parametrize("F,n,keep,msg", [(8, 6, 0, "keep ="), (8, 6, 7, "keep ="), (8, 6, 3, "odd dimension"),
                                          (9, 6, 2, "odd dimension"), (8, 5, 2, "odd dimension")],
                         ids=("keep 0", "keep K+1", "keep odd", "F odd", "3n odd"))
def test_pod_deflate_begin_refusals(F, n, keep, msg):
    rng = np.random.default_rng(9500 + F + n + keep)
    e, X, C, Bt = _refusal_engine(rng, F, n, 6)
    try:
        with pytest.raises(RuntimeError, match=msg):
            e.pod_deflate_begin(keep, Bt.data_ptr())
        assert np.array_equal(e.download_snapshots(), X) and np.array_equal(e.results_comps(), C)
        with pytest.raises(RuntimeError, match="without asb_pod_deflate_begin"):
            e.pod_deflate_end(0, 0)
        assert np.array_equal(e.download_snapshots(), X) and np.array_equal(e.results_comps(), C)
    finally:
        e.close()


def test_pod_deflate_end_refuses_last_above_k():
    rng = np.random.default_rng(9600)
    e, X, C, Bt = _refusal_engine(rng, 8, 6, 6)
    try:
        e.pod_deflate_begin(2, Bt.data_ptr())
        X1 = e.download_snapshots()
        with pytest.raises(RuntimeError, match="last ="):
            e.pod_deflate_end(7, 9)
        assert np.array_equal(e.download_snapshots(), X1) and np.array_equal(e.results_comps(), C)
        e.pod_deflate_end(6, 8)
        assert np.array_equal(e.results_comps(), np.concatenate([C[:2], C])) and np.array_equal(e.download_snapshots(), X)
    finally:
        e.close()


def _small_bases(rng, n):
    return [_orthonormal(rng, 3 * n, k).T.reshape(k, n, 3) for k in (6, 4, 4)]


@pytest.mark.parametrize("F2,n2", [(8, 6), (10, 8)], ids=("same shape", "other shape"))
def test_ingest_inside_an_open_level_drops_it(F2, n2):
    """new snapshots end an open level: they are what the context holds, asb_pod_deflate_end finds no level, and a cycle of
    levels on them gives the bits of a fresh engine (no row count and no deflated copy left over from the dropped level)"""
    rng = np.random.default_rng(9650 + F2)
    e, X, C, Bt = _refusal_engine(rng, 8, 6, 6)
    X2 = _two_groups(rng, F2, n2)
    bases = _small_bases(rng, n2)
    where = "ingest in a level F=%d n=%d" % (F2, n2)
    try:
        e.pod_deflate_begin(2, Bt.data_ptr())
        assert not np.array_equal(e.download_snapshots(), X)
        e.upload(X2, 0, n2)
        assert np.array_equal(e.download_snapshots(), X2), (where, "the context does not hold the new snapshots")
        with pytest.raises(RuntimeError, match="without asb_pod_deflate_begin"):
            e.pod_deflate_end(0, 0)
        assert np.array_equal(e.download_snapshots(), X2)
        got = _cycle(e, X2, bases, 2, where)
    finally:
        e.close()
    fresh = _engine(X2)
    try:
        ref = _cycle(fresh, X2, bases, 2, where + " fresh")
    finally:
        fresh.close()
    for a, b in zip(got, ref):
        assert np.array_equal(a, b), (where, "a cycle after the dropped level differs from the same cycle on a fresh engine")


def test_level_buffers_are_registered():
    """the level's deflated copy and kept rows belong to the context: an engine closed inside a level leaves nothing behind, and
    after asb_pod_deflate_end has released them a second cycle on the same engine repeats the first bit for bit"""
    rng = np.random.default_rng(9660)
    e, X, C, Bt = _refusal_engine(rng, 8, 6, 6)
    try:
        e.pod_deflate_begin(2, Bt.data_ptr())
        assert not np.array_equal(e.download_snapshots(), X)
    finally:
        e.close()
    bases = _small_bases(rng, 6)
    e = _engine(X)
    try:
        first = _cycle(e, X, bases, 2, "registered")
        again = _cycle(e, X, bases, 2, "registered again")
    finally:
        e.close()
    for a, b in zip(first, again):
        assert np.array_equal(a, b), "a second cycle on the same engine differs from the first"


@pytest.mark.parametrize("F,n,K", [(8, 6, 6), (70, 130, 64)], ids=("small", "big"))
def test_b_in_the_context_or_in_a_callers_tensor(F, n, K):
    """project -> rotate -> power and project -> rotate -> deflate_begin with B left in the context (B_dev = NULL throughout)
    give the bits of the same chain on a caller's tensor"""
    rng = np.random.default_rng(9700 + F)
    X = _two_groups(rng, F, n)
    Q = _orthonormal(rng, 3 * n, K).T.reshape(K, n, 3)
    out = {}
    for own in (False, True):
        for then in ("power", "deflate"):
            e = _engine(X)
            try:
                e.components_upload(Q)
                Bt = _tensor(size=K * F) if own else None
                ptr = Bt.data_ptr() if own else None
                B = e.pod_project(ptr)
                S = e.pod_rotate(ptr)
                Cn = e.results_comps()
                if then == "power":
                    e.pod_power(ptr)
                else:
                    e.pod_deflate_begin(2, ptr)
                out[own, then] = (B, S, Cn, e.results_comps(), e.download_snapshots())
            finally:
                e.close()
    for then in ("power", "deflate"):
        for a, b in zip(out[False, then], out[True, then]):
            assert np.array_equal(a, b), (then, "the context's B and a caller's tensor give different bits")
    assert not np.array_equal(out[True, "power"][3], out[True, "power"][2])
    assert not np.array_equal(out[True, "deflate"][4], X)


# ---------------------------------------------------------------------------------------------------------------- j. element-wise
def _within(phase, name, got, hi, terms, where):
    """|got - hi| <= 2 eps * (sum of the magnitudes of the model's terms), entry by entry"""
    assert np.isfinite(got).all(), (phase, name, where)
    err = np.abs(np.asarray(got, dtype=LD) - hi)
    worst = float((err / np.where(terms > 0, terms, 1)).max() / EPS) if err.size else 0.0
    print("%s %s %s: largest error %.2f eps of the terms (bound 2)" % (phase, name, where, worst))
    seen = _SEEN.setdefault((phase, name + " / eps"), [0.0, 0.0, 2.0])
    seen[0] = seen[1] = max(seen[0], worst)
    assert (err <= 2 * EPS * terms).all(), (phase, name, where, worst)


def _affine_cases(rng, n):
    """(inv_scale, add_mean, rowscale): with and without mean and rowscale, inv_scale no power of two"""
    rs = rng.uniform(0.5, 2.0, size=n)
    return [(1.0 / 3.7, True, None), (0.3, False, rs), (1.0 / 1.3, True, rs), (1.0, False, None)]


def _check_affine(F, n, where):
    rng = np.random.default_rng(10000 + 7 * F + n)
    X = 3.0 + rng.normal(size=(F, n, 3))
    e = _engine(X)
    try:
        e.center(1, True)
        mean = e.get_mean()
        for inv, add, rs in _affine_cases(rng, n):
            X0 = e.download_snapshots()
            e.snapshots_affine(inv, add, rs)
            m = mean if add else None
            _within("affine", "X", e.download_snapshots(), pm.affine(X0, inv, m, rs, LD), pm.affine_terms(X0, inv, m, rs),
                    "%s inv=%.3g mean=%d rowscale=%d" % (where, inv, add, rs is not None))
        # nothing landed in the padding columns [F, Fp): the Gram matrix reads whole padded rows
        Xd = e.download_snapshots()
        if F >= 3:
            A = pm.rows(Xd, LD)
            check("affine", "gram after", e.pod_gram(), pm.rows(Xd).T @ pm.rows(Xd), A.T @ A, where)
    finally:
        e.close()


@pytest.mark.parametrize("F", AFFINE_F)
def test_snapshots_affine(F):
    for n in AFFINE_N:
        _check_affine(F, n, "F=%d n=%d" % (F, n))


def test_snapshots_affine_grid_stride():
    """more rows than ROWS_PER_BLOCK * nblk_cap: the blocks of k_affine_rows go round their stride loop"""
    n = ROWS_PER_BLOCK * grid_cap() // 3 + 2
    assert 3 * n > ROWS_PER_BLOCK * grid_cap()
    _check_affine(3, n, "F=3 n=%d (grid stride)" % n)


def _check_post(K, n, where):
    rng = np.random.default_rng(11000 + 7 * K + n)
    X = 3.0 + rng.normal(size=(2, n, 3))
    im = rng.uniform(0.5, 2.0, size=n)
    e = _engine(X)
    try:
        e.center(1, True)
        mean = e.get_mean()
        for unscale, psf, inv_mass in [(True, 3.7, None), (False, 1.0, im), (True, 1.3, im), (False, 5.0, None)]:
            C = rng.normal(size=(K, n, 3))
            e.components_upload(C)
            out = e.components_post(unscale, psf, inv_mass)
            assert np.array_equal(out, e.results_comps())
            _within("comps_post", "C", out, pm.comps_post(C, unscale, psf, mean, inv_mass, LD),
                    pm.comps_post_terms(C, unscale, psf, mean, inv_mass), "%s unscale=%d psf=%.3g mass=%d" % (
                        where, unscale, psf, inv_mass is not None))
            if not unscale and inv_mass is None:
                assert np.array_equal(out, C), "nothing to do must change nothing"
    finally:
        e.close()


@pytest.mark.parametrize("K", (1, 5))
def test_components_post(K):
    for n in AFFINE_N:
        _check_post(K, n, "K=%d n=%d" % (K, n))


def test_components_post_grid_stride():
    """more entries than POST_PER_BLOCK * nblk_cap: the threads of k_comps_post go round their stride loop"""
    n, K = 1000, POST_PER_BLOCK * grid_cap() // 3000 + 2
    assert K * 3 * n > POST_PER_BLOCK * grid_cap()
    _check_post(K, n, "K=%d n=%d (grid stride)" % (K, n))


def test_mean_is_required():
    rng = np.random.default_rng(12000)
    X, C = rng.normal(size=(5, 4, 3)), rng.normal(size=(2, 4, 3))
    e = _engine(X)
    try:
        e.components_upload(C)
        with pytest.raises(RuntimeError, match="no mean on the device"):
            e.snapshots_affine(0.5, True)
        with pytest.raises(RuntimeError, match="no mean on the device"):
            e.components_post(True, 2.0, None)
        assert np.array_equal(e.download_snapshots(), X) and np.array_equal(e.results_comps(), C)
    finally:
        e.close()


@pytest.mark.parametrize("F,n", [(1, 1), (65, 100), (64, 2)])
def test_scale_affine_round_trip(F, n):
    """centre, scale by a, affine(1 / a, add the mean) restores the upload.  With d = x - mean: one rounding in d, one in a d, one
    in 1 / a, one in the product with it (each half an eps of |d|) and one in the sum (half an eps of |x| <= |d| + |mean|):
    2.5 eps |d| + 0.5 eps |mean| at the very worst, inside 2 eps (|d| + |mean|) wherever |d| <= 3 |mean|, which the inputs keep
    (asserted)"""
    rng = np.random.default_rng(13000 + F + n)
    X = 3.0 + rng.normal(size=(F, n, 3))
    a = 3.7
    e = _engine(X)
    try:
        e.center(1, True)
        mean = e.get_mean()
        e.scale(a)
        e.snapshots_affine(1.0 / a, True)
        back = e.download_snapshots()
    finally:
        e.close()
    d = np.abs(X.astype(LD) - mean[None])
    assert (d <= 3 * np.abs(mean)[None]).all(), "precondition"
    _within("affine", "back", back, X.astype(LD), d + np.abs(mean.astype(LD))[None], "F=%d n=%d" % (F, n))


def test_components_truncate():
    rng = np.random.default_rng(14000)
    C = rng.normal(size=(7, 5, 3))
    e = _basis_engine(C)
    try:
        for bad in (0, 8):
            with pytest.raises(RuntimeError):
                e.components_truncate(bad)
            assert e.K == 7 and np.array_equal(e.results_comps(), C)
        e.components_truncate(3)
        assert e.K == 3 and np.array_equal(e.results_comps(), C[:3])
        with pytest.raises(RuntimeError):
            e.components_truncate(4)
        e.orth_gram()
        check("orth_gram", "G", e.orth_gram_get(), pm.slice_grams(C[:3], np.float64), pm.slice_grams(C[:3], LD), "after truncate")
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- coverage
def test_cases_cover_the_edges():
    """The case tables themselves: both sides of every predicate, and the tails next to every switch."""
    for table in (GRAM_K, PROJ_K, QR_K):
        assert any(orth_syrk(K) for K in table) and any(not orth_syrk(K) and K > 64 for K in table)
        assert any(not orth_syrk(K) and K < 64 for K in table) and {63, 64, 65} <= set(table)
    assert 1 in GRAM_N and any(n % 16 for n in GRAM_N if n > 64)
    qr_n = [(K, n) for K in QR_K for n in (2 * K + 1, 2 * K + 2)]
    assert any(combine_rows_ok(K, n) for K, n in qr_n) and any(not combine_rows_ok(K, n) and orth_syrk(K) for K, n in qr_n)
    assert any(not combine_rows_ok(K, n) and K % 2 and K > 64 for K, n in qr_n)
    assert any(chol_one_block(K) for K in QR_K) and any(not chol_one_block(K) for K in QR_K) and {128, 129} <= set(QR_K)
    assert {78, 79} <= set(QR_K) and not chol_lds_optin(78) and chol_lds_optin(79)
    assert chol_lds_optin(128) and not chol_lds_optin(129)
    for table in (QR2_K, REFUSE_K):
        assert any(chol_lds_optin(K) for K in table) and any(not chol_one_block(K) for K in table)
    assert any(not chol_lds_optin(K) and chol_one_block(K) for K in REFUSE_K)
    basis = [(K, n, F, Kv) for F in BASIS_F for n in BASIS_N for K in BASIS_K for Kv in BASIS_KV(K) if Kv <= F]
    assert any(basis_gemm(*c) and c[3] == c[0] for c in basis) and any(basis_gemm(*c) and c[3] != c[0] for c in basis)
    for odd in range(4):            # the GEMM route lost to each of K, 3 n, F and eig_k alone being odd, at K >= 64
        assert any(c[0] >= 64 and [bool(v % 2) for v in (c[0], 3 * c[1], c[2], c[3])] == [i == odd for i in range(4)]
                   for c in basis), odd
    assert any(c[0] < 64 and not any(v % 2 for v in (c[0], 3 * c[1], c[2], c[3])) for c in basis)
    assert any(c[3] != c[0] for c in basis) and any(c[0] % 16 for c in basis) and any(c[0] == 16 for c in basis)
    assert any(F % 64 for F in BASIS_F) and 64 in BASIS_F and any(F > 128 for F in BASIS_F)
    assert 1 in PROJ_N and {n % 2 for n in PROJ_N} == {0, 1} and any(F % 64 == 0 for F in PROJ_F) and any(F % 64 for F in PROJ_F)
    rot = [(K, n) for K in ROT_K for n in (K + 1, K + 2)]
    assert any(combine_rows_ok(*c) for c in rot) and any(not combine_rows_ok(*c) and orth_syrk(c[0]) for c in rot)
    assert any(K % 2 for K in ROT_K) and 1 in ROT_K and 128 in ROT_K
    assert all(not (K % 2 or (K + 6) % 2 or (K + 2) % 2) for K in POWER_K) and any(K >= 64 for K in POWER_K)
    assert any(orth_syrk(s[2]) for s in DEFLATE_SHAPES) and any(not orth_syrk(s[2]) for s in DEFLATE_SHAPES)
    assert all(not (s[0] % 2 or (3 * s[1]) % 2) for s in DEFLATE_SHAPES)
    assert {F % 64 for F in AFFINE_F} >= {0, 1, 63} and 1 in AFFINE_F and 1 in AFFINE_N and any(n > 64 for n in AFFINE_N)
