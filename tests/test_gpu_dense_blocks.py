"""GPU (-m gpu): the dense f64 building blocks that most paths other than the greedy step rest on, called directly through
their test hooks (include/asb.h: asb_test_gemm_nn / _gemm_tn / _transpose / _sym_eig / _spd_inverse) at the shapes where they
branch.

* asb_gemm_nn (128 x 128 tiles, 16-deep stages, split-K over slabs summed by k_gemm_finish, the triangular form, C -= A B with
  the accumulators started from C): bit for bit against integer products, within 2 Kc eps (|A||B|) on floats, with NaN in the
  operands' padding and behind them, C's padding and a tail that must stay NaN, beta = 0 over a C of NaN / Inf, odd sizes refused,
  split-K sums repeatable bit for bit.
* The TN products: the symmetric 128-tile Gram kernel (asb_syrk_tn), its general form (asb_gemm_tn_big) and the one-wave-per-tile
  kernel with a strided operand and interleaved output (asb_gemm_tn_s): integer-exact, float-bounded, G exactly symmetric, the
  other two coordinate slices untouched, a row shard summed in the order of the whole (I_split).
* The transpose, the one-block Jacobi eigen-solver against numpy.linalg.eigh (random, exactly rank-deficient PSD, repeated
  eigenvalues, zero), the SPD inverse at the sizes that switch its path, its refusal of an indefinite matrix.
* Orthogonalisation with an odd K >= 64 (q_orthogonal against scipy's orth, constProj_orthogonal against economic QR).
* Every selectable form of this layer (ASB_GEMM_CINIT, ASB_DENSE_SYM, ASB_ORTH_SYRK, ASB_TRI_MULTISECT, ASB_TD_VARIANT,
  ASB_TD_SMALL_REG, ASB_BACKTRANSFORM_BLOCKED, the tridiagonalisation panels on small sizes) in a child process of its own: each
  switch is read once per process.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import relerr

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(np.float64).eps
TAIL = 37                   # NaN doubles behind every output buffer


def _cdiv(a, b):
    return (a + b - 1) // b


# ---- the slab rules of the wrappers (csrc/asb_dense.hip: asb_gemm_nn; csrc/asb_linalg.hip: asb_syrk_tn, asb_gemm_tn_s), to
# ---- name the branch each case takes
def nn_slabs(M, N, Kc, tri=0):
    tm, tn = _cdiv(M, 128), _cdiv(N, 128)
    S = 1
    if tm * tn < 512 and Kc >= 1024 and not tri:
        S = max(1, min(1024 // (tm * tn), Kc // 512, 32))
    slab = _cdiv(_cdiv(Kc, S), 16) * 16
    return _cdiv(Kc, slab), slab


def tn_s_slabs(R, I, J, I_split=0):
    tiles_s = _cdiv(I_split if I_split > 0 else I, 16) * _cdiv(J, 16)
    S = max(1, 4096 // max(tiles_s, 1))
    S = min(S, _cdiv(R, 64), 64)
    slab = _cdiv(_cdiv(R, S), 4) * 4
    return _cdiv(R, slab), slab


def big_slabs(R, tiles):
    S = _cdiv(8 * 512, tiles)
    S = min(S, max(_cdiv(R, 512), 1), 64)
    slab = max(_cdiv(_cdiv(R, S), 16) * 16, 16)
    return max(_cdiv(R, slab), 1), slab


def _status(exc):
    return str(exc.value).split("status ")[1].split(":")[0]


# ---------------------------------------------------------------------------------------------------------------- GEMM-NN
# (M, N, Kc, alpha, beta, tri).  alpha = -1, beta = 1 with one slab is the cinit form; beta = 0 runs over a C of NaN and Inf.
NN_CASES = [
    (2, 2, 2, 1.0, 0.0, 0), (16, 130, 14, 1.0, 0.0, 0), (126, 16, 18, 2.0, -3.0, 0), (128, 128, 16, 1.0, 1.0, 0),
    (130, 258, 130, -1.0, 1.0, 0), (258, 126, 1022, 1.0, 0.0, 0), (130, 130, 1024, 1.0, 0.0, 0), (130, 130, 1026, 2.0, -3.0, 0),
    (130, 130, 1026, -1.0, 1.0, 0), (2, 1002, 4098, 1.0, 0.0, 0), (1002, 1002, 4098, -1.0, 1.0, 0), (258, 2, 1026, 1.0, 0.0, 0),
    (1002, 130, 130, -1.0, 1.0, 0), (150004, 64, 288, 1.0, 0.0, 0),
    (258, 258, 130, 1.0, 0.0, 1), (1002, 1002, 18, -1.0, 1.0, 1), (130, 130, 1026, 1.0, 0.0, 1), (256, 256, 256, -1.0, 1.0, 1),
    (16, 16, 2, 2.0, -3.0, 1),
]
LDA_EXTRA, LDB_EXTRA, LDC_EXTRA = 6, 4, 2


def _nn_buffers(rng, M, N, Kc, beta, kind):
    A = np.full((M, Kc + LDA_EXTRA), np.nan)
    B = np.full((Kc, N + LDB_EXTRA), np.nan)
    C = np.full(M * (N + LDC_EXTRA) + TAIL, np.nan)
    Cm = C[:M * (N + LDC_EXTRA)].reshape(M, N + LDC_EXTRA)
    if kind == "int":
        A[:, :Kc] = rng.integers(-1000, 1001, size=(M, Kc))
        B[:, :N] = rng.integers(-1000, 1001, size=(Kc, N))
        Cm[:, :N] = rng.integers(-1000, 1001, size=(M, N))
    else:
        A[:, :Kc] = rng.uniform(-1, 1, size=(M, Kc))
        B[:, :N] = rng.uniform(-1, 1, size=(Kc, N))
        Cm[:, :N] = rng.uniform(-1, 1, size=(M, N))
    if beta == 0.0:         # BLAS: C is not read
        Cm[:, :N] = np.where(rng.random((M, N)) < 0.5, np.nan, np.inf * np.sign(rng.random((M, N)) - 0.7))
    return A, B, C, Cm


def _nn_call(e, A, B, C, M, N, Kc, alpha, beta, tri):
    return e.test_gemm_nn(A, B, C.copy(), N + LDC_EXTRA, M, N, Kc, alpha, beta, tri)


def _keep_mask(M, N, tri):
    """Where the result goes: everything, or the 128 x 128 tiles on and above the diagonal."""
    if not tri:
        return np.ones((M, N), bool)
    ti = np.arange(M)[:, None] // 128
    tj = np.arange(N)[None, :] // 128
    return tj >= ti


def check_nn(M, N, Kc, alpha, beta, tri, seed=0, repeat=False):
    """Integer-exact and float-bounded checks of one GEMM-NN shape (also the body of the ASB_GEMM_CINIT=0 child)."""
    from animsnapbases_amd import HipEngine
    rng = np.random.default_rng(seed + 7 * M + 131 * N + Kc)
    keep = _keep_mask(M, N, tri)
    e = HipEngine(0)
    try:
        for kind in ("int", "float"):
            A, B, C, Cm = _nn_buffers(rng, M, N, Kc, beta, kind)
            got = _nn_call(e, A, B, C, M, N, Kc, alpha, beta, tri)
            Gm = got[:M * (N + LDC_EXTRA)].reshape(M, N + LDC_EXTRA)
            assert np.isnan(got[M * (N + LDC_EXTRA):]).all(), "write behind C"
            assert np.isnan(Gm[:, N:]).all(), "write into C's row padding"
            res = Gm[:, :N]
            prod = A[:, :Kc] @ B[:, :N]
            base = Cm[:, :N] if beta != 0.0 else 0.0
            ref = alpha * prod + (beta * base if beta != 0.0 else 0.0)
            old = Cm[:, :N]
            # tiles below the diagonal of the triangular form keep what C held (NaN and Inf compare as themselves)
            below = ~keep
            if below.any():
                same = (res[below] == old[below]) | (np.isnan(res[below]) & np.isnan(old[below]))
                assert same.all(), "the triangular form wrote below the diagonal"
            r, f = res[keep], ref[keep]
            if kind == "int":
                bad = np.flatnonzero(r != f)
                assert bad.size == 0, ("integer product not exact", M, N, Kc, alpha, beta, tri, bad[:5].tolist(),
                                       r[bad[0]], f[bad[0]])
            else:
                mag = abs(alpha) * (np.abs(A[:, :Kc]) @ np.abs(B[:, :N])) + (abs(beta) * np.abs(old) if beta != 0.0 else 0.0)
                bound = 2 * (Kc + 2) * EPS * mag[keep]
                over = np.abs(r - f) - bound
                assert np.isfinite(r).all() and (over <= 0).all(), ("float product outside the rounding bound", M, N, Kc,
                                                                     alpha, beta, tri, float(np.nanmax(over)))
                if repeat:          # split-K sums in a fixed order: a second call gives the same bits
                    again = _nn_call(e, A, B, C, M, N, Kc, alpha, beta, tri)
                    assert np.array_equal(again, got, equal_nan=True), "two identical calls differ"
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("M,N,Kc,alpha,beta,tri", NN_CASES)
def test_gemm_nn_exact(M, N, Kc, alpha, beta, tri):
    check_nn(M, N, Kc, alpha, beta, tri, repeat=nn_slabs(M, N, Kc, tri)[0] > 1)


@gpu
def test_gemm_nn_refuses_odd_sizes():
    from animsnapbases_amd import HipEngine
    e = HipEngine(0)
    try:
        for M, N, Kc, lda, ldb, ldc, tri in [(3, 2, 2, 2, 2, 2, 0), (2, 3, 2, 2, 4, 4, 0), (2, 2, 3, 4, 2, 2, 0),
                                             (2, 2, 2, 3, 2, 2, 0), (2, 2, 2, 2, 3, 2, 0), (2, 2, 2, 2, 2, 3, 0),
                                             (4, 2, 2, 2, 2, 2, 1)]:
            A = np.ones((M, lda))
            B = np.ones((Kc, ldb))
            C = np.full(M * ldc + TAIL, np.nan)
            with pytest.raises(RuntimeError) as exc:
                e.test_gemm_nn(A, B, C, ldc, M, N, Kc, 1.0, 0.0, tri)
            assert _status(exc) == "-1", str(exc.value)
            assert np.isnan(C).all()
        # the same engine then multiplies correctly
        A = np.arange(4.0).reshape(2, 2)
        C = np.full(4 + TAIL, np.nan)
        e.test_gemm_nn(A, A, C, 2, 2, 2, 2)
        assert np.array_equal(C[:4].reshape(2, 2), A @ A) and np.isnan(C[4:]).all()
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- TN products
# (form, R, I, J, sx, I_split): form 0 = asb_gemm_tn_s (sx = 3: the coordinate-slice layout, output strides (3, 3 I)),
# 1 = asb_gemm_tn_big, 2 = asb_syrk_tn (J = I).
TN_CASES = [
    (2, 1, 2, 2, 1, 0), (2, 15, 127, 127, 1, 0), (2, 16, 128, 128, 1, 0), (2, 17, 129, 129, 1, 0), (2, 511, 130, 130, 1, 0),
    (2, 512, 257, 257, 1, 0), (2, 513, 3, 3, 1, 0), (2, 150003, 130, 130, 1, 0),
    (1, 1, 127, 129, 1, 0), (1, 17, 128, 2, 1, 0), (1, 513, 130, 257, 1, 0), (1, 150003, 64, 130, 1, 0), (1, 16, 1, 1, 1, 0),
    (0, 1, 1, 1, 3, 0), (0, 15, 16, 17, 3, 0), (0, 511, 65, 65, 1, 0), (0, 513, 130, 127, 3, 0), (0, 513, 130, 127, 3, 4000),
    (0, 4097, 1002, 64, 3, 0), (0, 150003, 40, 64, 3, 0), (0, 512, 129, 15, 1, 0),
]


def tn_branch(form, R, I, J, sx, I_split):
    if form == 0:
        return tn_s_slabs(R, I, J, I_split)
    if form == 1:
        return big_slabs(R, _cdiv(I, 128) * _cdiv(J, 128))
    nb = _cdiv(I, 128)
    return big_slabs(R, nb * (nb + 1) // 2)


def _tn_operands(rng, form, R, I, J, sx, kind):
    draw = (lambda s: rng.integers(-1000, 1001, size=s).astype(np.float64)) if kind == "int" else \
        (lambda s: rng.uniform(-1, 1, size=s))
    if form == 0:
        ldx = sx * I + 2
        X = np.full((R, ldx), np.nan)
        X[:, 0:sx * I:sx] = draw((R, I))            # the other slices of a row hold NaN: they must not leak
        Y = np.full((R, J + 3), np.nan)
    else:
        X = np.full((R, I + (I & 1) + 2), np.nan)   # even strides, NaN in columns I .. ld - 1
        X[:, :I] = draw((R, I))
        Y = np.full((R, J + (J & 1) + 4), np.nan) if form == 1 else None
    if Y is not None:
        Y[:, :J] = draw((R, J))
    Xv = X[:, 0:sx * I:sx] if form == 0 else X[:, :I]
    Yv = Xv if form == 2 else Y[:, :J]
    return X, Y, Xv, Yv


def _tn_call(e, form, X, Y, R, I, J, sx, I_split):
    if form == 0:
        out = np.full(3 * I * J + TAIL, np.nan) if sx == 3 else np.full(I * J + TAIL, np.nan)
        so_i, so_j = (3, 3 * I) if sx == 3 else (J, 1)
        e.test_gemm_tn(0, X, R, I, J, out, Y=Y, sx=sx, so_i=so_i, so_j=so_j, I_split=I_split)
        if sx == 3:
            idx = 3 * np.arange(I)[:, None] + 3 * I * np.arange(J)[None, :]
        else:
            idx = J * np.arange(I)[:, None] + np.arange(J)[None, :]
    else:
        out = np.full(I * J + TAIL, np.nan)
        e.test_gemm_tn(form, X, R, I, J, out, Y=Y)
        idx = J * np.arange(I)[:, None] + np.arange(J)[None, :]
    mask = np.ones(out.size, bool)
    mask[idx.ravel()] = False
    assert np.isnan(out[mask]).all(), "a write outside the I x J result (other coordinate slices, tail)"
    return out[idx]


def check_tn(form, R, I, J, sx, I_split, seed=0):
    from animsnapbases_amd import HipEngine
    rng = np.random.default_rng(seed + 17 * R + 5 * I + J + form)
    e = HipEngine(0)
    try:
        for kind in ("int", "float"):
            X, Y, Xv, Yv = _tn_operands(rng, form, R, I, J, sx, kind)
            got = _tn_call(e, form, X, Y, R, I, J, sx, I_split)
            ref = Xv.T @ Yv
            if kind == "int":
                bad = np.argwhere(got != ref)
                assert bad.size == 0, ("integer product not exact", form, R, I, J, bad[:5].tolist())
            else:
                bound = 2 * (R + 1) * EPS * (np.abs(Xv).T @ np.abs(Yv))
                over = np.abs(got - ref) - bound
                assert np.isfinite(got).all() and (over <= 0).all(), ("float product outside the rounding bound", form, R, I,
                                                                      J, float(np.nanmax(over)))
            if form == 2:
                assert np.array_equal(got, got.T), "the Gram matrix is not exactly symmetric"
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("form,R,I,J,sx,I_split", TN_CASES)
def test_gemm_tn_exact(form, R, I, J, sx, I_split):
    check_tn(form, R, I, J, sx, I_split)


@gpu
def test_gemm_tn_s_row_shard_sums_in_the_order_of_the_whole():
    """A row shard of the product with I_split = the whole's row count takes the whole's slabs: the same bits on floats."""
    from animsnapbases_amd import HipEngine
    R, I0, I1, J = 20000, 300, 40, 64
    assert tn_s_slabs(R, I1, J)[0] != tn_s_slabs(R, I0, J)[0] == tn_s_slabs(R, I1, J, I0)[0]
    rng = np.random.default_rng(5)
    X, Y, _, _ = _tn_operands(rng, 0, R, I0, J, 1, "float")
    e = HipEngine(0)
    try:
        whole = _tn_call(e, 0, X, Y, R, I0, J, 1, 0)
        shard = _tn_call(e, 0, X, Y, R, I1, J, 1, I0)
    finally:
        e.close()
    assert np.array_equal(shard, whole[:I1])


@gpu
def test_tn_kernels_refuse_odd_strides():
    """The 128-tile kernels stage double2 loads: an odd stride is refused, not read past its row."""
    from animsnapbases_amd import HipEngine
    e = HipEngine(0)
    try:
        X = np.ones((20, 5))
        Y = np.ones((20, 4))
        for form, Yarg in [(2, None), (1, Y)]:
            out = np.full(16 + TAIL, np.nan)
            with pytest.raises(RuntimeError) as exc:
                e.test_gemm_tn(form, X, 20, 4 if form == 1 else 3, 4 if form == 1 else 3, out, Y=Yarg)
            assert _status(exc) == "-1", str(exc.value)
            assert np.isnan(out).all()
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- transpose
TR_SIZES = [1, 31, 32, 33, 1000]


@gpu
def test_transpose_exact():
    from animsnapbases_amd import HipEngine
    rng = np.random.default_rng(1)
    e = HipEngine(0)
    try:
        for rows in TR_SIZES:
            for cols in TR_SIZES:
                A = rng.normal(size=(rows, cols))
                out = np.full(rows * cols + TAIL, np.nan)
                e.test_transpose(A, out)
                assert np.array_equal(out[:rows * cols].reshape(cols, rows), A.T), (rows, cols)
                assert np.isnan(out[rows * cols:]).all(), (rows, cols)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- Jacobi
EIG_SIZES = [1, 2, 3, 31, 32, 33, 64, 127, 128]
EIG_KINDS = ["random", "psd_rank_deficient", "repeated", "zero"]


def _eig_matrix(kind, n, rng):
    if kind == "random":
        B = rng.normal(size=(n, n))
        return 0.5 * (B + B.T)
    if kind == "psd_rank_deficient":       # integer W W^T: exactly rank n // 2 (a zero eigenvalue of multiplicity n - n // 2)
        W = rng.integers(-3, 4, size=(n, n // 2)).astype(np.float64)
        return W @ W.T
    if kind == "repeated":
        Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
        lam = np.array([3.0, 3.0, 3.0, -1.0, -1.0, 0.5, 2.0][:n] + list(rng.uniform(-2, 2, size=max(n - 7, 0))))
        A = (Q * lam) @ Q.T
        return 0.5 * (A + A.T)
    return np.zeros((n, n))


def _clusters(lam, tol):
    groups, cur = [], [0]
    for j in range(1, len(lam)):
        if lam[j - 1] - lam[j] <= tol:
            cur.append(j)
        else:
            groups.append(cur)
            cur = [j]
    groups.append(cur)
    return groups


def check_eig(n, kind, seed=0):
    from animsnapbases_amd import HipEngine
    rng = np.random.default_rng(seed + 101 * n + EIG_KINDS.index(kind))
    A = _eig_matrix(kind, n, rng)
    e = HipEngine(0)
    try:
        lam, V, st = e.test_sym_eig(A)
    finally:
        e.close()
    assert st == 0, "the Jacobi solver reports no convergence"
    ref_lam, ref_V = np.linalg.eigh(A)
    ref_lam, ref_V = ref_lam[::-1], ref_V[:, ::-1]
    nA = max(np.linalg.norm(A, 2), np.finfo(float).tiny)
    assert np.all(np.diff(lam) <= 0), "eigenvalues not descending"
    assert np.abs(lam - ref_lam).max() <= 8 * n * EPS * nA
    assert np.abs(A @ V - V * lam[None]).max() <= 8 * n * EPS * nA
    assert np.abs(V.T @ V - np.eye(n)).max() <= 8 * n * EPS
    # eigenvectors against LAPACK's: the projector onto each cluster of (nearly) equal eigenvalues, within eps |A| / gap
    tol = 1e-6 * nA
    for g in _clusters(ref_lam, tol):
        lo, hi = g[0], g[-1]
        gap = min(ref_lam[lo - 1] - ref_lam[lo] if lo else np.inf, ref_lam[hi] - ref_lam[hi + 1] if hi + 1 < n else np.inf)
        if not np.isfinite(gap):
            continue                     # the whole space
        P, Pr = V[:, g] @ V[:, g].T, ref_V[:, g] @ ref_V[:, g].T
        assert np.abs(P - Pr).max() <= 100 * n * EPS * nA / gap, (kind, n, g[:3], gap)


@gpu
@pytest.mark.parametrize("n", EIG_SIZES)
def test_jacobi_eig_vs_lapack(n):
    for kind in EIG_KINDS:
        check_eig(n, kind)


@gpu
def test_jacobi_eig_refuses_outside_one_block():
    from animsnapbases_amd import HipEngine
    e = HipEngine(0)
    try:
        with pytest.raises(RuntimeError) as exc:
            e.test_sym_eig(np.eye(129))
        assert _status(exc) == "-1"
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- SPD inverse
# 256: one pivot block of the symmetric form (Schur step, b2 = 128); 257 (padded to 272): pivot blocks 256 + 16; 528: 256 + 256 + 16
SPD_SIZES = [256, 257, 528]


def check_spd(n, seed=0):
    from animsnapbases_amd import HipEngine
    rng = np.random.default_rng(seed + n)
    B = rng.normal(size=(n, n))
    A = B @ B.T + 0.05 * n * np.eye(n)
    e = HipEngine(0)
    try:
        X = e.test_spd_inverse(A)
    finally:
        e.close()
    ref = np.linalg.inv(A)
    cond = np.linalg.cond(A)
    assert np.abs(X - ref).max() < 1e-12 * np.abs(ref).max() * cond
    assert np.abs(A @ X - np.eye(n)).max() < 50 * n * EPS * cond


def check_spd_refuses_indefinite(n, seed=0):
    """A symmetric indefinite matrix is refused (ASB_ERR_NUMERIC); the same engine then inverts an SPD one."""
    from animsnapbases_amd import HipEngine
    rng = np.random.default_rng(seed + n)
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    lam = rng.uniform(1, 2, size=n)
    lam[n // 3] = -0.5
    A = (Q * lam) @ Q.T
    A = 0.5 * (A + A.T)
    S = (Q * np.abs(lam)) @ Q.T
    S = 0.5 * (S + S.T)
    e = HipEngine(0)
    try:
        with pytest.raises(RuntimeError) as exc:
            e.test_spd_inverse(A)
        assert _status(exc) == "-5", str(exc.value)
        X = e.test_spd_inverse(S)
    finally:
        e.close()
    assert np.abs(S @ X - np.eye(n)).max() < 50 * n * EPS * np.linalg.cond(S)


@gpu
@pytest.mark.parametrize("n", SPD_SIZES)
def test_spd_inverse_path_switches(n):
    check_spd(n)


@gpu
@pytest.mark.parametrize("n", [100, 300])
def test_spd_inverse_refuses_indefinite(n):
    check_spd_refuses_indefinite(n)


# ---------------------------------------------------------------------------------------------------------------- odd K
def check_orth(K, seed=0):
    """q_orthogonal = scipy's SVD-based orth of the post-processed basis per coordinate (test_gpu_parity's pattern)."""
    from scipy.linalg import orth
    from test_gpu_parity import _param, _run
    rng = np.random.default_rng(seed + K)
    F, N = 150, 400
    verts = rng.uniform(-1, 1, size=(F, N, 3))
    snaps, comp = _run(verts, None, _param(vertPos_numComponents=K, q_orthogonal=True))
    pre_orth = comp.comps / snaps.pre_scale_factor + snaps.mean[None]
    comp.post_process_components()
    for l in range(3):
        ref = orth(pre_orth[:, :, l].T).T
        got = comp.comps[:, :, l]
        sg = np.sign(np.sum(got * ref, axis=1))
        assert relerr(got * sg[:, None], ref) < 1e-7, (K, l)
        assert np.allclose(got @ got.T, np.eye(K), atol=1e-10)


def check_qr(K, tmp, seed=0):
    """constProj_orthogonal = economic QR of the raw basis per coordinate, up to column signs."""
    import scipy.linalg as sla
    from test_gpu_parity import _run_constraints
    rng = np.random.default_rng(seed + K)
    frames = 0.1 + rng.normal(size=(150, 400, 3))
    ns, cc = _run_constraints(frames, K, True, tmp)
    raw = cc.comps.copy() / ns.pre_scale_factor + ns.mean[None]
    cc.post_process_components()
    for l in range(3):
        ref = sla.qr(raw[:, :, l].T, mode="economic")[0].T
        got = cc.comps[:, :, l]
        sg = np.sign(np.sum(got * ref, axis=1))
        assert relerr(got * sg[:, None], ref) < 1e-8, (K, l)
        assert np.allclose(got @ got.T, np.eye(K), atol=1e-11)


@gpu
@pytest.mark.parametrize("K", [64, 65, 127])
def test_orthogonal_odd_K_vs_scipy_orth(K):
    check_orth(K)


@gpu
def test_constraints_qr_odd_K(tmp_path):
    check_qr(65, tmp_path)


# ---------------------------------------------------------------------------------------------------------------- variants
EIGENSOLVER_SHAPES = [(65, 65), (130, 20), (777, 33), (1500, 64), (1700, 40)]
PANEL_SHAPES = [(600, 64), (777, 33), (1024, 40)]
TRIDIAG_CASES = [(3, 3, 1e-3, 3), (64, 10, 1e-4, 20), (65, 30, 1e-5, 65), (500, 40, 1e-6, 72), (1300, 60, 1e-5, 160)]


def _child_gemm_cinit():
    """ASB_GEMM_CINIT=0: C -= A B through the read-modify-write epilogue; the Gauss-Jordan sweeps are made of it."""
    cases = [c for c in NN_CASES if c[3] == -1.0 and c[4] == 1.0]
    for c in cases:
        check_nn(*c, seed=3)
    for n in (129, 257, 528):
        check_spd(n, seed=3)
    print("cinit off: %d products, 3 inverses OK" % len(cases))


def _child_dense_sym():
    """ASB_DENSE_SYM=0: the full-matrix Gauss-Jordan sweeps with k_block_inverse."""
    for n in (1, 100, 128, 129, 256, 257, 528):
        check_spd(n, seed=5)
    check_spd_refuses_indefinite(300, seed=5)
    print("dense sym off: 7 inverses, refusal OK")


def _child_orth_syrk():
    """ASB_ORTH_SYRK=0: the orth / QR Gram matrices and the joint rotation on the one-wave-per-tile kernel."""
    import tempfile
    for K in (64, 65):
        check_orth(K, seed=7)
        with tempfile.TemporaryDirectory() as tmp:
            check_qr(K, tmp, seed=7)
    print("orth syrk off: orth / qr OK")


def _child_tridiag():
    """ASB_TRI_MULTISECT=0: the eigenvalues of the tridiagonal solver by plain bisection (k_tri_bisect)."""
    import test_gpu_smalldense as t
    from animsnapbases_amd import HipEngine
    e = HipEngine(0)
    try:
        for c in TRIDIAG_CASES:
            t.test_tridiagonal_bisection_and_inverse_iteration(e, *c)
        t.test_tridiagonal_with_a_split_and_exact_multiplicity(e)
        import test_gpu_symeig as s                  # every tridiagonal family of symeig_cases.py, same bars
        for family in s.TRI_FAMILIES:
            s.check_tri_family(e, family)
    finally:
        e.close()
    print("bisection: %d cases, %d families OK" % (len(TRIDIAG_CASES) + 1, len(s.TRI_FAMILIES)))


def _child_eigensolver():
    """the symmetric eigen-solver's shapes (test_gpu_parity.test_device_symmetric_eigensolver) under the process's switches"""
    import test_gpu_parity as t
    shapes = PANEL_SHAPES if os.environ.get("ASB_TD_PANEL_MIN") else EIGENSOLVER_SHAPES
    for n, k in shapes:
        t.test_device_symmetric_eigensolver(n, k)
    if os.environ.get("ASB_BACKTRANSFORM_BLOCKED") == "0":
        import test_gpu_symeig as s                  # Q Z against the longdouble product at the (n, k) of the blocked route
        s.check_backtransform_all()
    print("eigensolver: %d shapes OK" % len(shapes))


def _child(body, env_over, timeout):
    env = dict(os.environ, **env_over)
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_dense_blocks as t; t.%s()" % (ROOT, HERE, body)
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=timeout)
    err = p.stderr.decode(errors="replace")
    assert p.returncode == 0, (p.returncode, err[-4000:])
    return p.stdout.decode()


VARIANTS = [
    ({"ASB_GEMM_CINIT": "0"}, "_child_gemm_cinit", "cinit off"),
    ({"ASB_DENSE_SYM": "0"}, "_child_dense_sym", "dense sym off"),
    ({"ASB_ORTH_SYRK": "0"}, "_child_orth_syrk", "orth syrk off"),
    ({"ASB_TRI_MULTISECT": "0"}, "_child_tridiag", "bisection"),
    ({"ASB_TD_VARIANT": "0"}, "_child_eigensolver", "eigensolver"),
    ({"ASB_TD_SMALL_REG": "0"}, "_child_eigensolver", "eigensolver"),
    ({"ASB_BACKTRANSFORM_BLOCKED": "0"}, "_child_eigensolver", "eigensolver"),
    ({"ASB_TD_PANEL_MIN": "600", "ASB_TD_PANEL_TAIL": "64"}, "_child_eigensolver", "eigensolver"),
]


@gpu
@pytest.mark.parametrize("env,body,word", VARIANTS, ids=[" ".join("%s=%s" % kv for kv in v[0].items()) for v in VARIANTS])
def test_selectable_forms(env, body, word):
    out = _child(body, env, timeout=300)
    assert word in out and "OK" in out, out


# ---------------------------------------------------------------------------------------------------------------- coverage
def test_cases_cover_the_edges():
    """The case tables themselves (no GPU needed): every edge value and branch at least once."""
    nn = NN_CASES
    assert {c[0] for c in nn} >= {2, 16, 126, 128, 130, 258, 1002} and {c[1] for c in nn} >= {2, 16, 126, 128, 130, 258, 1002}
    assert {c[2] for c in nn} >= {2, 14, 16, 18, 130, 1022, 1024, 1026, 4098}
    assert (150004, 64, 288) in {c[:3] for c in nn}                                   # the POD basis product
    split = [c for c in nn if nn_slabs(c[0], c[1], c[2], c[5])[0] > 1]
    assert split and any(c[2] % nn_slabs(c[0], c[1], c[2], c[5])[1] for c in split)    # split-K with a short last slab
    assert any(c[2] % 512 == 0 for c in split)                                         # ... and with whole slabs
    assert any(c[2] % 16 for c in nn if nn_slabs(*c[:3], c[5])[0] == 1)                # a partial last 16-deep stage
    assert any(c[5] and c[2] >= 1024 for c in nn)                                      # tri never splits
    assert any(c[5] and c[0] > 128 for c in nn)                                        # tiles below the diagonal
    cinit = [c for c in nn if c[3] == -1.0 and c[4] == 1.0]
    assert any(nn_slabs(c[0], c[1], c[2], c[5])[0] == 1 for c in cinit)                # cinit itself
    assert any(nn_slabs(c[0], c[1], c[2], c[5])[0] > 1 for c in cinit)                 # C - A B through the slab sum
    assert any(c[5] for c in cinit)                                                    # the Gauss-Jordan update's form
    assert any(c[4] == 0.0 and nn_slabs(*c[:3], c[5])[0] > 1 for c in nn)              # beta = 0 in k_gemm_finish
    assert any(c[4] == 0.0 and nn_slabs(*c[:3], c[5])[0] == 1 for c in nn)             # ... and in the tile epilogue
    assert any(c[4] not in (0.0, 1.0) for c in nn)
    tn = TN_CASES
    assert {c[1] for c in tn} >= {1, 15, 16, 17, 511, 512, 513, 150003}
    for form in (0, 1, 2):
        sizes = {c[2] for c in tn if c[0] == form} | {c[3] for c in tn if c[0] == form}
        assert sizes & {127, 129, 130, 257} and sizes & {1, 2, 3}                     # ragged around the 128 / 16 tiles
        assert any(tn_branch(*c)[0] > 1 for c in tn if c[0] == form)                  # split over slabs
        assert any(tn_branch(*c)[0] == 1 for c in tn if c[0] == form)                 # one slab
    assert {c[2] for c in tn if c[0] == 2} >= {127, 128, 129, 130, 257}
    s_cases = [c for c in tn if c[0] == 0 and c[4] == 3]
    assert any(tn_branch(*c)[0] == 1 for c in s_cases) and any(tn_branch(*c)[0] > 1 for c in s_cases)
    split_changed = [c for c in tn if c[0] == 0 and c[5] and tn_branch(*c)[0] != tn_branch(*c[:5], 0)[0]]
    assert split_changed                                                               # I_split changes the slabs
    assert set(TR_SIZES) == {1, 31, 32, 33, 1000}
    assert set(EIG_SIZES) >= {1, 2, 3, 31, 32, 33, 64, 127, 128}                      # odd n (dummy index), 256 / 1024 threads
    assert set(SPD_SIZES) >= {256, 257, 528}
    names = {k for v in VARIANTS for k in v[0]}
    assert names >= {"ASB_GEMM_CINIT", "ASB_DENSE_SYM", "ASB_ORTH_SYRK", "ASB_TRI_MULTISECT", "ASB_TD_VARIANT", "ASB_TD_SMALL_REG",
                     "ASB_BACKTRANSFORM_BLOCKED", "ASB_TD_PANEL_MIN", "ASB_TD_PANEL_TAIL"}
    assert {n for n, _ in PANEL_SHAPES} == {600, 777, 1024}
    assert any(n >= 256 and not n % 2 and not k % 2 for n, k in EIGENSOLVER_SHAPES)   # the blocked back-transform
