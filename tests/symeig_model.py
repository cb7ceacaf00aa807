"""High-precision model of the symmetric eigen-solver (csrc/asb_eig.hip + part 1 of csrc/asb_smalldense.hip) and the
measures its tests share (test_symeig_model_cpu.py, test_gpu_symeig.py).

* ``sturm_eigs``      -- all eigenvalues of a tridiagonal matrix by bisection on Sturm counts in numpy.longdouble;
* ``householder``     -- longdouble Householder tridiagonalisation (LAPACK's convention, the one of k_td_small);
* ``reference``       -- reference eigenpairs of a stored symmetric matrix: longdouble values, vectors from LAPACK made
                         accurate by one longdouble correction step between clusters;
* ``backtransform``   -- the longdouble product of the reflectors that asb_sym_tridiag leaves in A;
* ``invit_f64``       -- float64 transcription of k_tri_shifts + k_tri_invit, as they stood before the split-matrix repair
                         (``blocks=False``) and as they stand now (``blocks=True``);
* ``measure``         -- lam / res / unit / sub / ritz in units of eps max|lambda|, rank = cond(V).

Everything is evaluated from the STORED float64 matrix: no measure contains the error of forming the case."""
import numpy as np

LD = np.longdouble
EPS = 2.220446049250313e-16
CLUSTER_TOL = 1e-6          # values closer than this, relative to themselves, form one cluster
RANK_BAR = 2.0 ** 20        # cond(V): CholeskyQR2 behind it stops near eps^-1/2 = 2^26.5, 2^6 is left for what X adds


def dense_of(d, e):
    d, e = np.asarray(d, dtype=np.float64), np.asarray(e, dtype=np.float64)
    return np.diag(d) + (np.diag(e, 1) + np.diag(e, -1) if len(d) > 1 else 0.0)


# ---------------------------------------------------------------------------------------------------------------- bisection
def sturm_count(d, e, x):
    """#{eigenvalues of T(d, e) < x[i]} for every x[i] (longdouble; a zero pivot is replaced by a tiny negative one)."""
    d, e, x = np.asarray(d, dtype=LD), np.asarray(e, dtype=LD), np.asarray(x, dtype=LD)
    n = len(d)
    e2 = e * e
    tiny = np.finfo(LD).tiny * max(LD(1), e2.max() if n > 1 else LD(1))
    q = d[0] - x
    q = np.where(np.abs(q) < tiny, -tiny, q)
    cnt = (q < 0).astype(np.int64)
    for j in range(1, n):
        q = d[j] - x - e2[j - 1] / q
        q = np.where(np.abs(q) < tiny, -tiny, q)
        cnt += q < 0
    return cnt


def sturm_eigs(d, e):
    """All eigenvalues of T(d, e), ASCENDING, by longdouble bisection down to the last bit of the bracket."""
    d, e = np.asarray(d, dtype=LD), np.asarray(e, dtype=LD)
    n = len(d)
    if n == 1:
        return d.copy()
    r = np.zeros(n, dtype=LD)
    r[:-1] += np.abs(e)
    r[1:] += np.abs(e)
    nrm = max(np.abs(d - r).max(), np.abs(d + r).max())
    if nrm == 0:
        return np.zeros(n, dtype=LD)
    lo = np.full(n, (d - r).min() - nrm * LD(1e-15), dtype=LD)
    hi = np.full(n, (d + r).max() + nrm * LD(1e-15), dtype=LD)
    idx = np.arange(n)
    for _ in range(200):
        mid = (lo + hi) / 2
        live = (mid > lo) & (mid < hi)
        if not live.any():
            break
        up = sturm_count(d, e, mid) > idx
        hi = np.where(live & up, mid, hi)
        lo = np.where(live & ~up, mid, lo)
        if ((hi - lo) <= LD(2.0) ** -70 * nrm).all():
            break
    return (lo + hi) / 2


# ---------------------------------------------------------------------------------------------------------------- Householder
def householder(A):
    """A = Q T Q^T in longdouble: (d, e, V, tau) with H_j = I - tau_j v_j v_j^T, v_j[j + 1] = 1 (rows of V), tau_j = 0
    when A[j + 2:, j] is already zero -- the convention of k_td_small."""
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    V, tau = np.zeros((max(n - 2, 0), n), dtype=LD), np.zeros(max(n - 2, 0), dtype=LD)
    for j in range(n - 2):
        x = A[j + 1:, j].copy()
        alpha, sigma = x[0], (x[1:] * x[1:]).sum()
        if sigma == 0:
            continue
        beta = -np.copysign(np.sqrt(alpha * alpha + sigma), alpha)
        t = (beta - alpha) / beta
        v = x / (alpha - beta)
        v[0] = 1
        V[j, j + 1:], tau[j] = v, t
        B = A[j + 1:, j + 1:]
        p = t * (B @ v)
        w = p - (t / 2) * (p @ v) * v
        A[j + 1:, j + 1:] = B - np.outer(v, w) - np.outer(w, v)
        A[j + 1, j] = A[j, j + 1] = beta
        A[j + 2:, j] = A[j, j + 2:] = 0
    return np.diag(A).copy(), np.diag(A, 1).copy(), V, tau


def reflectors_of(A_stored):
    """(V, tau) from the matrix asb_sym_tridiag has overwritten: v_j in row j, columns j + 1 .., v_j[j + 1] = 1; tau_j = 2 / |v_j|^2
    (an orthogonal reflector has no other), 0 where the stored tail is zero (k_td_small: sigma == 0)."""
    A = np.asarray(A_stored, dtype=LD)
    n = A.shape[0]
    V, tau = np.zeros((max(n - 2, 0), n), dtype=LD), np.zeros(max(n - 2, 0), dtype=LD)
    for j in range(n - 2):
        tail = A[j, j + 2:]
        if not np.any(tail):
            continue
        V[j, j + 1], V[j, j + 2:] = 1, tail
        tau[j] = 2 / (V[j] @ V[j])
    return V, tau


def backtransform(V, tau, Z):
    """Q Z = H_0 H_1 ... H_{n-3} Z in longdouble."""
    X = np.array(Z, dtype=LD)
    for j in range(len(tau) - 1, -1, -1):
        if tau[j] != 0:
            X -= np.outer(tau[j] * V[j], V[j] @ X)
    return X


# ---------------------------------------------------------------------------------------------------------------- reference
def clusters(lam_desc, tol=CLUSTER_TOL):
    """Runs of consecutive (descending) values closer to their neighbour than tol times their own size -- the rule of
    test_pod_clustered_spectrum_vs_lapack_on_A -- or than 64 eps max|lambda|, below which float64 does not tell them apart."""
    lam_desc = np.asarray(lam_desc, dtype=np.float64)
    n, scale = len(lam_desc), np.abs(lam_desc).max() if len(lam_desc) else 0.0
    out, k = [], 0
    while k < n:
        j = k + 1
        while j < n and lam_desc[j - 1] - lam_desc[j] <= max(tol * max(abs(lam_desc[j - 1]), abs(lam_desc[j])), 64 * EPS * scale):
            j += 1
        out.append((k, j))
        k = j
    return out


def reference(A):
    """(lam, U): eigenvalues DESCENDING in longdouble (Householder + bisection, both longdouble) and longdouble vectors whose
    CLUSTER subspaces are accurate: LAPACK's vectors, one first-order correction between different clusters
    (X_ij = B_ij / (B_jj - B_ii), B = U^T A U), then orthonormalised in longdouble (_orthonormal)."""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    d, e, _, _ = householder(A)
    lam = sturm_eigs(d, e)[::-1].copy()
    U = np.linalg.eigh(A)[1][:, ::-1].astype(LD)
    Al = A.astype(LD)
    for _ in range(2):
        B = U.T @ Al @ U
        cl = np.empty(n, dtype=np.int64)
        for c, (a, b) in enumerate(clusters(lam)):
            cl[a:b] = c
        diff = np.diag(B)[None, :] - np.diag(B)[:, None]
        other = cl[:, None] != cl[None, :]
        X = np.where(other, B / np.where(other, diff, LD(1)), LD(0))
        U = U + U @ X
        U = _orthonormal(U)
    return lam, U


def _orthonormal(U):
    """Columns that are orthonormal to float64 rounding -> to longdouble rounding: U <- U (I - (U^T U - I) / 2), three times (each
    step squares the defect).  Columns that are not even nearly orthonormal (a rank-deficient V) come back as they are."""
    U = np.array(U, dtype=LD)
    I = np.eye(U.shape[1], dtype=LD)
    for _ in range(3):
        D = U.T @ U - I
        if not np.abs(D).max() < 0.5:
            break
        U = U - U @ (D / 2)
    return U


# ---------------------------------------------------------------------------------------------------------------- measures
def measure(A, lam_got, V, ref_lam, ref_U, k):
    """The measures of a result (lam_got: all n values descending or None; V: n x k) against the reference (ref_U: at least
    the columns of every cluster that starts inside the k leading values), in units of
    eps max|lambda| (1 where the matrix is zero); 'rank' is cond(V) itself; 'cut' the number of the k leading values that sit in a
    cluster cut by k (skipped by 'sub')."""
    if callable(A):
        mv = A                                  # A V for a longdouble V, where the matrix is too large to hold in longdouble
    else:
        Al = np.asarray(A, dtype=np.float64).astype(LD)
        mv = lambda X: Al @ X
    n = len(ref_lam)
    scale = LD(np.abs(np.asarray(ref_lam, dtype=np.float64)).max())
    unit_ = EPS * (scale if scale > 0 else LD(1))
    out = {}
    if lam_got is not None:
        lam_got = np.asarray(lam_got, dtype=np.float64)
        out["lam"] = float(np.abs(lam_got.astype(LD) - ref_lam[:len(lam_got)]).max() / unit_)
        out["descending"] = bool(np.all(np.diff(lam_got) <= 0))
    if V is None:
        return out
    Vl = np.asarray(V, dtype=LD)
    lam_k = (lam_got[:k].astype(LD) if lam_got is not None else ref_lam[:k])
    R = mv(Vl) - Vl * lam_k[None, :]
    out["res"] = float(np.sqrt((R * R).sum(axis=0)).max() / unit_)
    out["unit"] = float(np.abs(np.sqrt((Vl * Vl).sum(axis=0)) - 1).max() / EPS)
    V64 = np.asarray(V, dtype=np.float64)
    sv = np.linalg.svd(V64, compute_uv=False)
    out["rank"] = float(sv[0] / sv[-1]) if sv[-1] > 0 else float("inf")
    Q = np.linalg.qr(V64)[0].astype(LD)
    Q = _orthonormal(Q)                         # orthonormal to longdouble accuracy (when V has full rank)
    H = (Q.T @ mv(Q)).astype(np.float64)
    ritz = np.linalg.eigvalsh(0.5 * (H + H.T))[::-1]
    out["ritz"] = float(np.abs(ritz.astype(LD) - ref_lam[:k]).max() / unit_)
    sub, cut = 0.0, 0
    for a, b in clusters(ref_lam):
        if a >= k:
            break
        if b > k:
            # a cluster cut by k: which of its vectors come out is not determined, but span(V) still has to lie inside the
            # reference subspace of everything down to the cluster's end
            cut = k - a
            if b < n and b <= ref_U.shape[1]:
                Ub = ref_U[:, :b]
                D = Q - Ub @ (Ub.T @ Q)
                sub = max(sub, float(np.sqrt((D * D).sum(axis=0)).max() * (ref_lam[b - 1] - ref_lam[b]) / unit_))
            break
        gap = min(ref_lam[a - 1] - ref_lam[a] if a else np.inf, ref_lam[b - 1] - ref_lam[b] if b < n else np.inf)
        if not np.isfinite(float(gap)):
            continue                            # the whole space
        Uc = ref_U[:, a:b]
        D = Uc - Q @ (Q.T @ Uc)
        sub = max(sub, float(np.sqrt((D * D).sum(axis=0)).max() * gap / unit_))
    out["sub"], out["cut"] = sub, cut
    return out


# ---------------------------------------------------------------------------------------------------------------- transcription
M32 = np.uint64(0xFFFFFFFF)
SPLIT = 2.0                 # ASB_TRI_SPLIT of asb_smalldense.hip: |e[j]| <= SPLIT eps |T| ends a block


def gershgorin_norm(d, e):
    """TRI_BNORM of k_tri_prepare: the larger end of the Gershgorin interval, in float64 as the kernel forms it"""
    d, e = np.asarray(d, dtype=np.float64), np.asarray(e, dtype=np.float64)
    r = np.zeros(len(d))
    r[:-1] += np.abs(e)
    r[1:] += np.abs(e)
    return max(abs((d - r).min()), abs((d + r).max()))


def split_starts(d, e):
    """first rows of the blocks k_tri_blocks finds, and n"""
    thr = SPLIT * EPS * gershgorin_norm(d, e)
    return [0] + [j for j in range(1, len(d)) if abs(e[j - 1]) <= thr] + [len(d)]


def invit_f64(d, e, lam_desc, k, blocks):
    """float64 transcription of k_tri_shifts + k_tri_invit.  blocks=False: the routine before the split-matrix repair (the whole
    matrix from one constant start vector, coinciding shifts pushed apart everywhere).  blocks=True: the repaired one -- blocks
    from |e[j]| <= 2 eps |T| (split_starts), a start direction of its own and a reachable growth criterion for every
    vector whose shift was pushed, re-orthogonalisation inside every chain of pushed shifts (k_tri_reorth), every eigenvalue owned by the block whose Sturm count holds it, shifts pushed apart within a block, the
    iteration on the block alone.  (Z n x k, number of flagged vectors)."""
    d, e = np.asarray(d, dtype=np.float64), np.asarray(e, dtype=np.float64)
    lam_desc = np.asarray(lam_desc, dtype=np.float64)
    n = len(d)
    gl = min(d[j] - (abs(e[j - 1]) if j else 0.0) - (abs(e[j]) if j < n - 1 else 0.0) for j in range(n))
    gu = max(d[j] + (abs(e[j - 1]) if j else 0.0) + (abs(e[j]) if j < n - 1 else 0.0) for j in range(n))
    bnorm = max(abs(gl), abs(gu))
    starts = split_starts(d, e) if blocks else [0, n]
    if blocks and len(starts) > 2:
        # owner of every eigenvalue: the blocks' own spectra (LAPACK here, bisection on the device), merged descending with
        # the device's tie rule (equal values: the later slot first)
        val, own = np.empty(n), np.empty(n, dtype=np.int64)
        for b in range(len(starts) - 1):
            s0, s1 = starts[b], starts[b + 1]
            val[s0:s1] = np.linalg.eigvalsh(dense_of(d[s0:s1], e[s0:s1 - 1])) if s1 - s0 > 1 else d[s0]
            own[s0:s1] = b
        order = sorted(range(n), key=lambda i: (-val[i], -i))
        lam_desc, owner = val[order], own[order]
    else:
        owner = np.zeros(n, dtype=np.int64)
    floor_ = 1e-3 * EPS * bnorm
    sh, last, nxt, fac = np.empty(k), {}, {}, {}
    for j in range(k):
        pert = 10.0 * EPS * abs(lam_desc[j]) + floor_
        p = last.get(owner[j], -1)
        push = p >= 0 and sh[p] - lam_desc[j] < pert
        sh[j] = sh[p] - pert if push else lam_desc[j]
        if push:
            nxt[p] = j
        last[owner[j]] = j
    Z, bad = np.zeros((n, k)), 0
    eps3 = EPS * (bnorm if bnorm > 0.0 else 1.0)
    big = np.finfo(np.float64).max
    with np.errstate(all="ignore"):
        for v in range(k):
            s0, s1 = starts[owner[v]], starts[owner[v] + 1]
            m = s1 - s0
            if m == 1:
                Z[s0, v] = 1.0
                continue
            x1 = sh[v]
            eps4 = m * eps3
            uk = eps4 / np.sqrt(float(m))
            rv1, rv2, rv3, rv4, sw = np.zeros(m), np.zeros(m), np.zeros(m), np.zeros(m), np.zeros(m, dtype=bool)
            dd, ee = d[s0:s1], e[s0:s1 - 1]
            u, vv = dd[0] - x1, ee[0]
            for i in range(1, m):
                ei = ee[i - 1]
                enext = ee[i] if i < m - 1 else 0.0
                if abs(ei) >= abs(u) and ei != 0.0:
                    xu = u / ei
                    rv4[i], rv1[i - 1] = xu, ei
                    r2 = dd[i] - x1
                    rv2[i - 1], rv3[i - 1] = r2, enext
                    u, vv, sw[i] = vv - xu * r2, -xu * enext, True
                else:
                    if u == 0.0:
                        u = eps3
                    xu = ei / u
                    rv4[i], rv1[i - 1], rv2[i - 1], rv3[i - 1] = xu, u, vv, 0.0
                    u, vv, sw[i] = dd[i] - x1 - xu * vv, enext, False
            if u == 0.0:
                u = eps3
            rv1[m - 1], rv2[m - 1], rv3[m - 1] = u, 0.0, 0.0
            dlt = abs(lam_desc[v] - x1)
            grow = 0.1 * eps4 / dlt if blocks and 10.0 * dlt > eps4 else 1.0
            x = np.full(m, uk)
            if blocks and dlt != 0.0:                               # a pushed shift: a start direction of its own
                h = (np.arange(m, dtype=np.uint64) * 2654435761 + v * 2246822519 + 374761393) & M32
                h ^= h >> 15
                h = (h * 2246822519) & M32
                h ^= h >> 13
                h = (h * 3266489917) & M32
                h ^= h >> 16
                x = uk * ((h >> 8).astype(np.float64) * (1.0 / 8388608.0) - 1.0)
            ok, extra = False, 0
            for its in range(8):
                bu = bv = nrm = 0.0
                for i in range(m - 1, -1, -1):
                    t = (x[i] - bu * rv2[i] - bv * rv3[i]) / rv1[i]
                    x[i], bv, bu = t, bu, t
                    nrm += abs(t)
                if ok and not nrm < big:
                    break
                if nrm >= grow:
                    ok = True
                    if extra == 2:
                        break
                    extra += 1
                elif ok or its >= 5:
                    break
                if nrm == 0.0 or nrm != nrm:
                    x[:] = 0.0
                    x[its % m] = eps4
                else:
                    x *= eps4 / nrm
                for i in range(1, m):
                    t = x[i]
                    if sw[i]:
                        t, x[i - 1] = x[i - 1], x[i]
                    x[i] = t - rv4[i] * x[i - 1]
            s2 = float(np.sum(x * x))
            good = s2 > 0.0 and s2 < big
            bad += (not ok) or (not good)
            Z[s0:s1, v] = x * (1.0 / np.sqrt(s2) if good else 0.0)
            fac[v] = (rv1, rv2, rv3, rv4, sw, eps4)
        if blocks:                                                  # k_tri_reorth: inside every chain of pushed shifts
            for v0 in range(k):
                if sh[v0] != lam_desc[v0] or v0 not in nxt:
                    continue
                s0, s1 = starts[owner[v0]], starts[owner[v0] + 1]
                if s1 - s0 == 1:
                    continue
                members, t = [v0], nxt[v0]
                while True:
                    z = Z[s0:s1, t].copy()
                    rv1, rv2, rv3, rv4, sw, eps4 = fac[t]
                    good = True
                    for step in range(2):
                        for s_ in members:
                            z -= (Z[s0:s1, s_] @ z) * Z[s0:s1, s_]
                        s2 = float(z @ z)
                        good = good and s2 > 0.0 and s2 < big
                        z *= ((eps4 if step == 0 else 1.0) / np.sqrt(s2)) if good else 0.0
                        if step == 1:
                            break
                        for i in range(1, s1 - s0):
                            x_ = z[i]
                            if sw[i]:
                                x_, z[i - 1] = z[i - 1], z[i]
                            z[i] = x_ - rv4[i] * z[i - 1]
                        bu = bv = 0.0
                        for i in range(s1 - s0 - 1, -1, -1):
                            x_ = (z[i] - bu * rv2[i] - bv * rv3[i]) / rv1[i]
                            z[i], bv, bu = x_, bu, x_
                    Tb = dense_of(d[s0:s1], e[s0:s1 - 1])
                    r_new = float(np.sum((Tb @ z - lam_desc[t] * z) ** 2))
                    r_old = float(np.sum((Tb @ Z[s0:s1, t] - lam_desc[t] * Z[s0:s1, t]) ** 2))
                    if good and r_new <= 16.0 * max(r_old, eps3 * eps3):    # else: not one eigenspace, k_tri_invit's vector stays
                        Z[s0:s1, t] = z
                    members.append(t)
                    if t not in nxt:
                        break
                    t = nxt[t]
    return lam_desc, Z, bad


# ---------------------------------------------------------------------------------------------------------------- LAPACK
def lapack_tri(d, e):
    """scipy.linalg.eigh_tridiagonal (stemr; where stemr reports no convergence -- it does on some glued Wilkinson matrices --
    the QL driver stev): (lam descending, vectors in that order)."""
    from scipy.linalg import eigh_tridiagonal
    if len(d) == 1:
        return np.array(d, dtype=np.float64), np.ones((1, 1))
    try:
        lam, V = eigh_tridiagonal(d, e)
    except np.linalg.LinAlgError:
        lam, V = eigh_tridiagonal(d, e, lapack_driver="stev")
    return lam[::-1].copy(), V[:, ::-1].copy()


def lapack_dense(A):
    """numpy.linalg.eigh for the pairs, scipy.linalg.hessenberg for T: (lam descending, vectors, d, e)."""
    from scipy.linalg import hessenberg
    lam, V = np.linalg.eigh(A)
    H = hessenberg(A) if A.shape[0] > 2 else A
    return lam[::-1].copy(), V[:, ::-1].copy(), np.diag(H).copy(), np.diag(H, 1).copy()


def tri_error(d, e, ref_lam):
    """'tri': the eigenvalues of T(d, e) (longdouble bisection) against the reference of A, in units of eps max|lambda|"""
    scale = LD(np.abs(np.asarray(ref_lam, dtype=np.float64)).max())
    return float(np.abs(sturm_eigs(d, e)[::-1] - ref_lam).max() / (EPS * (scale if scale > 0 else LD(1))))
