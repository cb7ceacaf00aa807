"""Cases of the symmetric eigen-solver's tests (test_symeig_model_cpu.py, test_gpu_symeig.py): tridiagonal families for
bisection + inverse iteration, dense families for the whole chain, the permuted 1-2-1 matrix at the sizes where the
tridiagonalisation and the back-transformation change kernels, and the constants of csrc/asb_eig.hip that decide those routes.

A case is a dict: family, label, the matrix (d, e or A) and the vector counts ks.  Every family has a predicate (PREDICATES)
that test_symeig_model_cpu.py asserts on each of its cases, so that a case cannot drift to the friendly side unnoticed."""
import numpy as np

from symeig_model import LD

TRI_SIZES = [1, 2, 3, 63, 64, 65, 130]
DENSE_SIZES = [3, 4, 5, 64, 65, 130]
SCALES = [(-400, "x2^-400"), (400, "x2^400")]
GLUES = [1e-2, 1e-6, 1e-10, 1e-13, 3e-14]
AT_SIZE = [256, 258, 322, 1537, 4200, 5089, 6785, 10177]


def ks_for(n):
    """k = 1, 63, 64, 65, n: both sides of the 64-thread blocks of k_tri_invit"""
    return sorted({k for k in (1, 63, 64, 65, n) if 1 <= k <= n})


# ---------------------------------------------------------------------------------------------------------------- tridiagonal
def toeplitz121(n):
    return np.full(n, 2.0), np.ones(max(n - 1, 0))


def toeplitz121_pairs(n, idx):
    """Closed-form eigenpairs of the 1-2-1 matrix in longdouble: lambda_j = 2 + 2 cos(j pi / (n + 1)), j = 1 .. n (descending),
    v_j[i] = sqrt(2 / (n + 1)) sin((i + 1) j pi / (n + 1)); idx: 0-based positions in the descending order."""
    pi = LD(4) * np.arctan(LD(1))
    j = np.asarray(idx, dtype=LD) + 1
    lam = 2 + 2 * np.cos(j * pi / (n + 1))
    i = np.arange(1, n + 1, dtype=LD)
    V = np.sqrt(LD(2) / (n + 1)) * np.sin(np.outer(i, j) * pi / (n + 1))
    return lam, V


def wilkinson(m):
    """W(2m+1)+: d = |m - i|, e = 1"""
    return np.abs(np.arange(-m, m + 1)).astype(np.float64), np.ones(2 * m)


def glued(m, copies, glue):
    d0, e0 = wilkinson(m)
    d = np.tile(d0, copies)
    e = np.concatenate([np.concatenate([e0, [glue]]) for _ in range(copies)])[:-1]
    return d, e


def period3(n):
    return np.tile([2.0, 1.0, 3.0], n // 3 + 1)[:n], np.tile([0.5, 0.5, 0.0], n // 3 + 1)[:n - 1]


def identical_blocks(m, copies, seed=5):
    rng = np.random.default_rng(seed + m)
    d0, e0 = rng.normal(size=m), 0.3 + rng.random(m - 1)
    d = np.tile(d0, copies)
    e = np.concatenate([np.concatenate([e0, [0.0]]) for _ in range(copies)])[:-1]
    return d, e


def graded(n):
    """diagonal 2^0 .. 2^-60 by powers of two, off-diagonals a quarter of the geometric mean of their neighbours (a power of two)"""
    p = np.round(np.linspace(0, 60, n)).astype(int) if n > 1 else np.zeros(1, dtype=int)
    d = 2.0 ** -p
    e = 0.25 * 2.0 ** -((p[:-1] + p[1:] + 1) // 2)
    return d.astype(np.float64), e.astype(np.float64)


def gram_like(n):
    from test_gpu_smalldense import _gram_like_tridiag
    d, e, _ = _gram_like_tridiag(n, max(1, min(n, n // 4 + 1)), 1e-5, seed=n)
    return d, e


def _tri(family, label, d, e, ks=None):
    d, e = np.asarray(d, dtype=np.float64), np.asarray(e, dtype=np.float64)
    return {"family": family, "label": label, "d": d, "e": e, "ks": ks if ks is not None else ks_for(len(d))}


def tri_cases():
    out = []
    rng = np.random.default_rng(2024)
    for n in TRI_SIZES:
        out.append(_tri("toeplitz", "toeplitz-%d" % n, *toeplitz121(n)))
        out.append(_tri("multiple", "cI-%d" % n, np.full(n, 0.75), np.zeros(n - 1)))
        out.append(_tri("multiple", "diag-repeated-%d" % n, np.tile([3.0, -1.0, 3.0, 0.5], n // 4 + 1)[:n], np.zeros(n - 1)))
        out.append(_tri("zero", "zero-%d" % n, np.zeros(n), np.zeros(n - 1)))
        out.append(_tri("tiny_e", "e=1e-9-%d" % n, 1.0 + np.arange(n) / n, np.full(n - 1, 1e-9)))
        out.append(_tri("graded", "graded-%d" % n, *graded(n)))
        if n >= 3:
            out.append(_tri("gram", "gram-%d" % n, *gram_like(n)))
        if n >= 63:
            out.append(_tri("split", "period3-%d" % n, *period3(n)))
    out.append(_tri("split", "period3-30", *period3(30)))
    for m, c in ((32, 2), (65, 2), (21, 3), (43, 3)):
        out.append(_tri("split", "blocks-%dx%d" % (m, c), *identical_blocks(m, c)))
    out.append(_tri("split", "six", [2.0, 1.0, 3.0, 2.0, 1.0, 5.0], [0.5, 0.5, 0.0, 0.5, 0.25]))
    d0, e0 = identical_blocks(32, 1)
    out.append(_tri("split", "order1-between", np.concatenate([d0, [d0[3]], d0]), np.concatenate([e0, [0.0, 0.0], e0])))
    out.append(_tri("split", "order1-between-eig", np.concatenate([d0, [np.linalg.eigvalsh(np.diag(d0) + np.diag(e0, 1) + np.diag(e0, -1))[-1]], d0]),
                    np.concatenate([e0, [0.0, 0.0], e0])))
    for m in (10, 30, 50):
        out.append(_tri("wilkinson", "W%d+" % (2 * m + 1), *wilkinson(m)))
    for m, c in ((10, 5), (10, 12), (30, 4)):
        for g in GLUES:
            d, e = glued(m, c, g)
            out.append(_tri("glued", "W%d+x%d-glue%g" % (2 * m + 1, c, g), d, e, ks=sorted({1, c, 2 * c, 64, 65, len(d)} & set(range(1, len(d) + 1)))))
    del rng
    # every non-zero family also at the two ends of the exponent range that the unscaled sums of squares allow
    base = {c["label"]: c for c in out}
    for lab in ("toeplitz-65", "cI-64", "diag-repeated-65", "e=1e-9-63", "graded-65", "gram-65", "period3-30", "blocks-32x2", "blocks-21x3",
                "order1-between", "W21+", "W21+x5-glue1e-10"):
        c = base[lab]
        for p, name in SCALES:
            out.append(_tri(c["family"], "%s %s" % (lab, name), np.ldexp(c["d"], p), np.ldexp(c["e"], p), ks=c["ks"]))
    return out


def tri_predicate(c, ref_lam):
    """True when the case is what its family says (ref_lam: longdouble eigenvalues, descending)."""
    d, e, fam, n = c["d"], c["e"], c["family"], len(c["d"])
    scale = float(np.abs(ref_lam).max())
    if fam == "toeplitz":
        lam, V = toeplitz121_pairs(n, np.arange(n))
        T = (np.diag(d) + (np.diag(e, 1) + np.diag(e, -1) if n > 1 else 0)).astype(LD)
        s = LD(2) ** int(round(np.log2(scale / float(np.abs(lam).max()))))          # the case's power-of-two scaling
        return bool(np.abs(T @ V - V * (lam * s)[None]).max() <= 64 * np.finfo(LD).eps * scale and np.abs(ref_lam - lam * s).max() <= 64 * np.finfo(LD).eps * scale)
    if fam in ("multiple", "zero"):
        return bool(not np.any(e) and (fam == "zero") == (not np.any(d)) and (n < 3 or len(np.unique(d)) < n))
    if fam == "tiny_e":
        return bool(np.all(e / d[0] == 1e-9) and np.all(np.diff(d) > 0))
    if fam == "graded":
        return bool(n == 1 or (d.max() / d.min() == 2.0 ** 60 and np.all(e != 0)))
    if fam == "gram":
        return bool(np.all(e != 0) and ref_lam[-1] > -1e-12 * scale)
    if fam == "split":
        gaps = np.abs(np.diff(ref_lam))
        shared = c["label"].startswith("six") or gaps.min() <= 4 * 2.3e-16 * scale            # a value shared by two blocks
        return bool(np.any(e == 0) and np.any(e != 0) and shared)
    if fam == "wilkinson":
        return bool(np.all(e != 0) and ref_lam[0] - ref_lam[1] <= 1e-12 * scale)
    if fam == "glued":
        copies = int(c["label"].split("x")[1].split("-")[0])
        return bool(np.all(e != 0) and ref_lam[0] - ref_lam[copies - 1] <= 1e-10 * scale + 4 * e.min())
    return False


# ---------------------------------------------------------------------------------------------------------------- dense
def _sym(A):
    return 0.5 * (A + A.T)


def _perm(A, rng):
    p = rng.permutation(A.shape[0])
    return A[np.ix_(p, p)]


def kron_gram(r, m, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(m, m + 10))
    return np.kron(np.eye(r), _sym(X @ X.T))


def _dense(family, label, A, ks, **extra):
    A = np.ascontiguousarray(A, dtype=np.float64)
    assert np.array_equal(A, A.T)
    return dict({"family": family, "label": label, "A": A, "ks": sorted(set(ks))}, **extra)


def dense_cases():
    out = []
    for n in DENSE_SIZES:
        rng = np.random.default_rng(700 + n)
        kk = [1, max(1, n // 4), n]
        out.append(_dense("random", "random-%d" % n, _sym(rng.normal(size=(n, n))), kk))
        r = max(1, n // 4)
        B = rng.normal(size=(n, r))
        out.append(_dense("lowrank", "lowrank-%d" % n, _sym(B @ B.T + 1e-7 * _sym(rng.normal(size=(n, n)))), [1, r]))   # k outside the noise floor
        Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
        s = 0.85 ** np.arange(n)
        if n >= 4:
            s[1:4] = s[1]
        if n >= 64:
            s[8:16] = s[8]
        out.append(_dense("plateau", "plateau-%d" % n, _sym((Q * s) @ Q.T), [1, n] + ([4] if n >= 4 else []) + ([16] if n >= 64 else [])))
        c = np.exp(-np.minimum(np.arange(n), n - np.arange(n)) / 3.0)
        out.append(_dense("circulant", "circulant-%d" % n, c[(np.arange(n)[:, None] - np.arange(n)[None, :]) % n], [1, n] + ([3, 2 * (n // 4) + 1] if n > 5 else [])))
        for r_ in (2, 3):
            m = n // r_
            if m >= 2 and n != 5:
                K = kron_gram(r_, m, 900 + n)
                ks_ = [r_, r_ * max(1, m // 2), r_ * m]
                out.append(_dense("kron", "kron%d-%d" % (r_, r_ * m), K, ks_, zero_e=[m * b - 1 for b in range(1, r_)]))
                if m >= 21:
                    out.append(_dense("kron_perm", "kron%d-perm-%d" % (r_, r_ * m), _perm(K, rng), ks_))
        out.append(_dense("diagonal", "cI-%d" % n, 0.75 * np.eye(n), [1, n], t_is_a=True))
        out.append(_dense("diagonal", "diag-%d" % n, np.diag(np.tile([3.0, -1.0, 3.0, 0.5, 7.0], n // 5 + 1)[:n]), kk, t_is_a=True))
        d, e = rng.normal(size=n), rng.normal(size=n - 1)
        out.append(_dense("tridiagonal", "tridiagonal-%d" % n, np.diag(d) + np.diag(e, 1) + np.diag(e, -1), kk, t_is_a=True))
        Aw = np.diag(1.0 + np.arange(n))
        Aw[0, 1:] = Aw[1:, 0] = rng.normal(size=n - 1)
        out.append(_dense("arrowhead", "arrowhead-%d" % n, Aw, kk))
        u = rng.integers(-9, 10, size=n).astype(np.float64)
        u[0] = 3.0
        out.append(_dense("rank1", "rank1-%d" % n, np.outer(u, u), [1]))
        Ai = _sym(rng.normal(size=(n, n)))
        Ai[n // 2, :] = Ai[:, n // 2] = 0.0
        out.append(_dense("isolated", "isolated-%d" % n, Ai, kk))
        out.append(_dense("zero", "zero-%d" % n, np.zeros((n, n)), [1, n]))
    seen = set()
    out = [c for c in out if not (c["label"] in seen or seen.add(c["label"]))]        # n = 64 and 65 give the same kron orders
    base = {c["label"]: c for c in out}
    for lab in ("random-65", "kron2-64", "kron3-perm-63", "plateau-64", "circulant-65", "arrowhead-5"):
        c = base[lab]
        for p, name in SCALES:
            extra = {k: v for k, v in c.items() if k in ("zero_e", "t_is_a")}
            out.append(_dense(c["family"], "%s %s" % (lab, name), np.ldexp(c["A"], p), c["ks"], **extra))
    return out


def dense_predicate(c, ref_lam):
    A, fam, n = c["A"], c["family"], c["A"].shape[0]
    scale = float(np.abs(ref_lam).max())
    gaps = np.abs(np.diff(ref_lam))
    off = A - np.diag(np.diag(A))
    if fam == "random":
        return bool(ref_lam[0] > 0 > ref_lam[-1])
    if fam == "lowrank":
        r = max(1, n // 4)
        return bool(ref_lam[r - 1] > 1e3 * abs(ref_lam[r]) and np.any(ref_lam[r:] != 0))
    if fam == "plateau":
        return bool(n < 4 or (ref_lam[1] - ref_lam[3] <= 1e-13 * scale and (n < 64 or ref_lam[8] - ref_lam[15] <= 1e-13 * scale)))
    if fam == "circulant":
        return bool(np.array_equal(A[0], np.roll(A[1], -1)) and np.sum(gaps <= 1e-13 * scale) >= (n - 1) // 2)     # a looping animation: pairs
    if fam in ("kron", "kron_perm"):
        r = int(c["label"][4])
        m = n // r
        blockdiag = not np.any(A * (1 - np.kron(np.eye(r), np.ones((m, m)))))
        return bool(np.sum(gaps <= 4 * 2.3e-16 * scale) >= (r - 1) * m and blockdiag == (fam == "kron"))
    if fam == "diagonal":
        return bool(not np.any(off))
    if fam == "tridiagonal":
        return bool(not np.any(np.triu(A, 2)) and np.all(np.diag(A, 1) != 0))
    if fam == "arrowhead":
        return bool(not np.any(off[1:, 1:]) and np.all(A[0, 1:] != 0))
    if fam == "rank1":
        return bool(np.array_equal(A, np.round(A)) and np.linalg.matrix_rank(A) == 1)
    if fam == "isolated":
        return bool(not np.any(A[n // 2]) and np.count_nonzero(A) == (n - 1) ** 2)
    if fam == "zero":
        return bool(not np.any(A))
    return False


# ---------------------------------------------------------------------------------------------------------------- at size
# constants mirrored from csrc/asb_eig.hip (test_cases_cover_the_edges of test_symeig_model_cpu.py recomputes the routes)
TD_T, TD_CW, TDP_NB, TDP_T, TB_NB = 1024, 1024, 32, 512, 64
PANEL_MIN, PANEL_TAIL = 1536, 512
AT_SIZE_KS = {256: [2, 3], 258: [2, 3], 322: [2, 3], 1537: [2, 3], 4200: [2, 3], 5089: [3], 6785: [3], 10177: [1, 2]}
NO_PANEL = 10177            # this size also with ASB_TD_PANEL_MIN=0: the two-launch loop from the first column


def routes(n, k, panels=True, blocked=True):
    """Which kernels asb_sym_tridiag and asb_sym_backtransform take at (n, k): mirrors sym_tridiag / sym_backtransform_dev."""
    use_panels = panels and n >= PANEL_MIN and (n + TDP_T + 4 * TDP_NB) * 8 <= 150 * 1024
    js = 0
    if use_panels:
        while n - js > max(PANEL_TAIL, 64) + TDP_NB:
            js += TDP_NB
    small, chunks = set(), set()
    for j in range(js - 1, n - 2):
        rows_left = n - (j + 1)
        small.add("reg4" if rows_left <= 4 * TD_T else "reg8" if rows_left <= 8 * TD_T else "small")
        if j + 1 <= n - 3:
            chunks.add((n - (j + 2) + TD_CW - 1) // TD_CW)
    out = {"panels": js // TDP_NB, "panel_chunks": (n + TD_CW - 1) // TD_CW if use_panels else 0, "small": small, "update_chunks": max(chunks) if chunks else 0}
    if blocked and n % 2 == 0 and k % 2 == 0 and n >= 4 * TB_NB:
        nrefl = n - 2
        out.update(back="blocked", groups=(nrefl + TB_NB - 1) // TB_NB, last_group=nrefl % TB_NB or TB_NB)
    else:
        out.update(back="wave", wpb=min(4, (160 * 1024 - 1024) // (8 * n)))
    return out


def perm121(n, seed=11):
    """The 1-2-1 matrix under a fixed random permutation: A[p[i], p[j]] = T[i, j] -- integer entries, closed-form eigenpairs
    (toeplitz121_pairs, rows permuted by p) at any n.  Returns (A, p)."""
    p = np.random.default_rng(seed + n).permutation(n)
    A = np.zeros((n, n))
    A[p, p] = 2.0
    A[p[:-1], p[1:]] = 1.0
    A[p[1:], p[:-1]] = 1.0
    return A, p


def perm121_matvec(p, V):
    """A V for A = perm121 without forming A (any dtype of V)."""
    X = V[p]
    Y = 2 * X
    Y[:-1] += X[1:]
    Y[1:] += X[:-1]
    out = np.empty_like(Y)
    out[p] = Y
    return out


def toeplitz121_lam(n):
    pi = LD(4) * np.arctan(LD(1))
    return 2 + 2 * np.cos(np.arange(1, n + 1, dtype=LD) * pi / (n + 1))


def perm121_reference(n, p, k):
    """(all eigenvalues descending, the leading k + 64 reference vectors) of perm121(n) in longdouble, closed form"""
    nv = min(n, k + 64)
    _, V = toeplitz121_pairs(n, np.arange(nv))
    U = np.empty_like(V)
    U[p] = V
    return toeplitz121_lam(n), U


# ---------------------------------------------------------------------------------------------------------------- bars
# LAPACK's worst figure per family and measure on these very cases (scipy.linalg.eigh_tridiagonal; numpy.linalg.eigh and
# scipy.linalg.hessenberg), in units of eps max|lambda|, rounded up to three digits;
# test_lapack_error_is_what_the_bars_were_derived_from measures them again.
LAPACK_TRI = {
    'toeplitz': {'lam': 3.1, 'res': 16.3, 'unit': 1.95, 'sub': 0.981, 'ritz': 10.4},
    'multiple': {'lam': 0, 'res': 0, 'unit': 0, 'sub': 0, 'ritz': 0},
    'zero': {'lam': 0, 'res': 0, 'unit': 0, 'sub': 0, 'ritz': 0},
    'tiny_e': {'lam': 2.52, 'res': 2.53, 'unit': 0.447, 'sub': 0.085, 'ritz': 10.6},
    'graded': {'lam': 2.68, 'res': 4.3, 'unit': 1.53, 'sub': 3.9, 'ritz': 4.02},
    'gram': {'lam': 7.14, 'res': 9.35, 'unit': 2.5, 'sub': 3.55, 'ritz': 6.05},
    'split': {'lam': 21, 'res': 22.9, 'unit': 2.33, 'sub': 1.38, 'ritz': 17.5},
    'wilkinson': {'lam': 5.54, 'res': 6.94, 'unit': 1.44, 'sub': 1.74, 'ritz': 8.13},
    'glued': {'lam': 13.5, 'res': 15, 'unit': 16.8, 'sub': 3.17, 'ritz': 14.3},
}
LAPACK_DENSE = {
    'random': {'lam': 3, 'res': 6.65, 'unit': 5.42, 'sub': 1.69, 'ritz': 16.3, 'tri': 1.02},
    'lowrank': {'lam': 1.91, 'res': 4.11, 'unit': 4.99, 'sub': 1.58, 'ritz': 4.25, 'tri': 1.99},
    'plateau': {'lam': 3.97, 'res': 6.85, 'unit': 6.78, 'sub': 2.95, 'ritz': 4.74, 'tri': 2.33},
    'circulant': {'lam': 3.47, 'res': 6.16, 'unit': 8.43, 'sub': 1.09, 'ritz': 9.42, 'tri': 1.87},
    'diagonal': {'lam': 0, 'res': 0, 'unit': 0, 'sub': 0, 'ritz': 0, 'tri': 0},
    'tridiagonal': {'lam': 5.22, 'res': 6.74, 'unit': 6, 'sub': 0.842, 'ritz': 16.3, 'tri': 0},
    'arrowhead': {'lam': 2.94, 'res': 4.17, 'unit': 4.48, 'sub': 0.855, 'ritz': 9.75, 'tri': 2.99},
    'rank1': {'lam': 1.97, 'res': 2.94, 'unit': 1.12, 'sub': 2.24, 'ritz': 0.00113, 'tri': 1.97},
    'isolated': {'lam': 2.45, 'res': 5.74, 'unit': 4.67, 'sub': 1.67, 'ritz': 17.1, 'tri': 2.28},
    'zero': {'lam': 0, 'res': 0, 'unit': 0, 'sub': 0, 'ritz': 0, 'tri': 0},
    'kron': {'lam': 4.76, 'res': 5.45, 'unit': 5.59, 'sub': 1.63, 'ritz': 13.9, 'tri': 1.91},
    'kron_perm': {'lam': 5.97, 'res': 6.33, 'unit': 7.29, 'sub': 1.56, 'ritz': 7.92, 'tri': 1.76},
}
LAPACK_AT_SIZE = {
    256: {'lam': 1.6, 'res': 4.3, 'unit': 0.74, 'sub': 0.186, 'ritz': 1.01, 'tri': 1.24},
    258: {'lam': 2.21, 'res': 3.94, 'unit': 1.1, 'sub': 0.229, 'ritz': 1.68, 'tri': 1.38},
    322: {'lam': 2.35, 'res': 4.59, 'unit': 0.684, 'sub': 0.225, 'ritz': 1.88, 'tri': 1.12},
    1537: {'lam': 2.14, 'res': 4.32, 'unit': 2.11, 'sub': 0.0933, 'ritz': 0.45, 'tri': 2.08},
    4200: {'lam': 1.92, 'res': 8.73, 'unit': 1.34, 'sub': 0.142, 'ritz': 0.916, 'tri': 3.43},
}


def bar(literal):
    """the project's rule: eight times LAPACK's worst, and never below 16"""
    return max(8.0 * literal, 16.0)


def at_size_bar(n, q):
    """above n = 4200 LAPACK was not run: its figure at 4200 times sqrt(n / 4200) (independent rounding errors: a random walk)"""
    lit = LAPACK_AT_SIZE[n][q] if n in LAPACK_AT_SIZE else LAPACK_AT_SIZE[4200][q] * np.sqrt(n / 4200.0)
    return bar(lit)
