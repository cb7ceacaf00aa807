"""Reference model of the snapshot preparation (csrc/asb_snapshots.hip, posSnapshots.standarize), shared by
test_prep_model_cpu.py and test_gpu_prep.py.

Two kinds of model:

* ORDER models in float64, for what the device defines to the bit:
  - an element of the tensor: one multiply (m x), at most one subtract (the product comes back from LDS or from memory, so the
    compiler cannot contract it into the subtraction), one multiply by a;
  - the mean of rest shape 1 (k_center): lane f of a wave adds row[f], row[f + 64], ... from 0 in that order, the lanes are added
    by the xor butterfly 32, 16, 8, 4, 2, 1 (wave_sum), the result is divided by F.
  Nothing else is modelled to the bit.
* a numpy.longdouble model of every sum, evaluated on float64 inputs AS STORED: the sums are compared with longdouble sums of
  the order model's tensor, so the elementwise roundings are on both sides and a bound covers the summation alone.

Bounds.  u = 2^-53.  A float64 sum of terms t_i, however bracketed, has the error  <= depth u sum |t_i|  to first order, depth =
the most additions any one term takes part in.  A kernel that forms a serial chain of c terms per lane, s tree stages and a final
serial pass over p partials has depth <= c + s + p; the bound used is (c + s + p + 2) u sum |t_i|  (`sum_bound`), the 2 covering
the second-order terms and the final rounding.  Terms that are themselves rounded add their roundings per term (`extra`): a
square x x one, a squared deviation (x - mu)^2 three (the rounding of x - mu enters the square twice).  c, s, p, read from
the kernels (grid = the launch's block count, at most nblk_cap):

  k_center / k_sqdev + k_sum (`depth_rows`): a lane adds ceil(F / 64) entries of a row; wave_sum 6 stages; a wave adds its
    ceil(rows / (4 grid)) rows; (sh0 + sh1) + (sh2 + sh3) 2 stages; k_sum: a thread adds ceil(grid / 256) partials, wave_sum 6
    stages, then 4 wave results serially.  c = ceil(F / 64) + ceil(rows / (4 grid)) + ceil(grid / 256), s = 14, p = 4.
  k_transpose_first + k_sum_pairs (`depth_fused`): a thread adds 4 ceil(F / 32) entries; block_sum: 6 stages + 4 waves serially;
    k_sum_pairs: a thread adds ceil(nb / 1024) strips, 6 stages, 16 waves serially.  c = 4 ceil(F / 32) + ceil(nb / 1024), s = 12, p = 20.
  k_scale_energy, per vertex (`depth_e0`, `depth_rowsum`): E0: two chains of 3 ceil(Fp / 128) squares per lane, e0 + e1, 6 stages:
    c = 3 ceil(Fp / 128), s = 7, p = 0, one rounding per square.  Row sum s_d: q.x + q.y (1 stage), a chain of ceil(Fp / 128), 6
    stages: c = ceil(Fp / 128), s = 7.  m_v = (s_0^2 + s_1^2 + s_2^2) (1 / F): three squares, two adds, the rounded 1 / F and the
    product, 6 roundings of the whole, on top of 2 |s_d| ds_d + ds_d^2 from each row sum's own bound ds_d.
    EV = max(E0 - m_v, 0) gets the sum of the two bounds plus one rounding of the difference (max(., 0) is 1-Lipschitz).
  block totals of k_scale_energy + k_e0_finish (`depth_totals`): a wave adds ceil(n / (4 grid)) vertices, 2 stages; a thread of
    k_e0_finish adds ceil(grid / 256) partials, 6 stages, 2 stages.  c = ceil(n / (4 grid)) + ceil(grid / 256), s = 10, p = 0.  The
    maximum is exact.
  k_ev_moments (`depth_moments`): a thread adds ceil(n / 1024) values, 6 stages, 16 serially: c = ceil(n / 1024), s = 6, p = 16.
  k_stream<T, E2> without the update (`depth_stream`; the projection mode's own energy pass, csrc/asb_kernels.h): a thread adds
    3 E2 terms x^2 + y^2 (1 stage each), wave_sum 6 stages, then the T / 64 waves of a vertex serially: c = 3 E2, s = 7,
    p = T / 64, one rounding per square; T and E2 are what pick_cfg gives for the row length (asb_test_pick_cfg).

  mean_frac = S_m / S_E and ev_cv2 = n S_2 / S_1^2 - 1 get their bounds by first-order propagation through the quotient
  (`quotient_bound`, `cv2_bound`) plus the roundings of the host arithmetic.
  var: on the two-pass branch var = sqdev(mu) / count, where an error dmu of mu adds count dmu^2 (second order) to the sum; on
  the one-sweep branch var = S2 / count - mu^2 additionally carries 2 u (1 + mu^2 / var) relative (three host roundings of
  quantities of size mu^2 + var).  pre_scale_factor = 1 / sqrt(var): half the relative bound of var plus two roundings.
"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def pad16(F):
    return (F + 15) // 16 * 16


def _cdiv(a, b):
    return -(-int(a) // int(b))


# ------------------------------------------------------------------------------------------------ order models (float64)
def wave_sum64(v):
    """(R, 64) -> (R): the xor butterfly of wave_sum (every lane ends with the same value)"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    assert (v == v[:, :1]).all()
    return v[:, 0]


def lane_sum(rows):
    """(R, F) -> (R): k_center's order: lane f adds row[f], row[f + 64], ... from 0, then the butterfly"""
    R, F = rows.shape
    v = np.zeros((R, 64))
    for k0 in range(0, F, 64):
        chunk = rows[:, k0:k0 + 64]
        v[:, :chunk.shape[1]] = v[:, :chunk.shape[1]] + chunk
    return wave_sum64(v)


def order_tensor(X, massL, v0, n_loc, code, subtract):
    """-> (tensor (F, n_loc, 3), rest shape (n_loc, 3)) as the device defines them, float64"""
    X = np.asarray(X, dtype=np.float64)
    F = X.shape[0]
    Y = X[:, v0:v0 + n_loc].copy()
    if massL is not None:
        Y = Y * np.asarray(massL, dtype=np.float64)[v0:v0 + n_loc, None]
    if code == 0:
        mean = Y[0].copy()
    else:
        mean = (lane_sum(Y.reshape(F, n_loc * 3).T.copy()) / float(F)).reshape(n_loc, 3)
    if subtract:
        Y = Y - mean[None]
    return Y, mean


def vertex_major(Y):
    """(F, n, 3) -> (n, 3, Fp) with zero padding: the device layout"""
    F, n, _ = Y.shape
    out = np.zeros((n, 3, pad16(F)))
    out[:, :, :F] = Y.transpose(1, 2, 0)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


# ------------------------------------------------------------------------------------------------ longdouble model
def ld_prepare(X, massL, v0, n_loc, code, subtract):
    """the preparation in longdouble on the float64 inputs as stored -> (tensor, rest shape)"""
    Y = np.asarray(X, dtype=np.float64)[:, v0:v0 + n_loc].astype(LD)
    if massL is not None:
        Y = Y * np.asarray(massL, dtype=np.float64)[v0:v0 + n_loc, None].astype(LD)
    mean = Y[0].copy() if code == 0 else Y.sum(axis=0) / LD(Y.shape[0])
    if subtract:
        Y = Y - mean[None]
    return Y, mean


def ld_sums(T, mu=0.0):
    """T float64 (any shape) -> dict of longdouble: sum, sum |x|, sum x^2, sum (x - mu)^2 for the float64 mu as stored"""
    t = np.asarray(T, dtype=np.float64).astype(LD)
    d = t - LD(np.float64(mu))
    return dict(sum=t.sum(), abs=np.abs(t).sum(), sq=(t * t).sum(), sqdev=(d * d).sum(), count=t.size)


def ld_std(T):
    """population standard deviation of all entries (np.std) in longdouble, two passes -> (mu, var, std)"""
    t = np.asarray(T, dtype=np.float64).astype(LD)
    mu = t.sum() / LD(t.size)
    var = ((t - mu) ** 2).sum() / LD(t.size)
    return mu, var, np.sqrt(var)


def ld_energies(T):
    """T (F, n, 3) float64, the SCALED tensor as the device holds it -> dict of longdouble per-vertex arrays:
    E0 = sum x^2, s (n, 3) row sums, A (n, 3) = sum |x| per row, mv = sum_d s_d^2 / F, EV = max(E0 - mv, 0)"""
    t = np.asarray(T, dtype=np.float64).astype(LD)
    F = t.shape[0]
    E0 = (t * t).sum(axis=(0, 2))
    s = t.sum(axis=0)
    A = np.abs(t).sum(axis=0)
    mv = (s * s).sum(axis=1) / LD(F)
    EV = np.maximum(E0 - mv, LD(0))
    return dict(E0=E0, s=s, A=A, mv=mv, EV=EV, F=F)


def ev_integer_model(T):
    """integer data whose sums fit 53 bits: E0 and S = sum_d s_d^2 are exact whatever the order or contraction, so
    m_v = fl(S fl(1 / F)) and EV = fl(E0 - m_v) (or 0) are defined to the bit -> (E0, m_v, EV) float64"""
    ti = np.asarray(T, dtype=np.float64)
    assert (ti == np.rint(ti)).all()
    ti = ti.astype(np.int64)
    F = ti.shape[0]
    E0 = (ti * ti).sum(axis=(0, 2))
    s = ti.sum(axis=0)
    S = (s * s).sum(axis=1)
    assert np.abs(ti).max(initial=0) < 2 ** 20 and E0.max(initial=0) < 2 ** 53 and S.max(initial=0) < 2 ** 53
    E0f, Sf = E0.astype(np.float64), S.astype(np.float64)
    m = Sf * (1.0 / float(F))
    return E0f, m, np.where(E0f > m, E0f - m, 0.0)


def fits53(T, extra=()):
    """integer tensor: sum |x|, sum x^2 (hence every partial sum of either) fit 53 bits; asserted in int64"""
    ti = np.asarray(T, dtype=np.float64)
    if not (ti == np.rint(ti)).all() or np.abs(ti).max(initial=0) >= 2 ** 20:
        return False
    ti = ti.astype(np.int64)
    return bool(np.abs(ti).sum() < 2 ** 53 and (ti * ti).sum() < 2 ** 53 and all(abs(int(e)) < 2 ** 53 for e in extra))


# ------------------------------------------------------------------------------------------------ depths and bounds
def row_grid(n_loc, cap):
    return min(_cdiv(3 * n_loc, 4), cap)


def energy_grid(n_loc, cap):
    return min(_cdiv(n_loc, 4), cap)


def depth_rows(F, n_loc, cap):
    g = row_grid(n_loc, cap)
    return _cdiv(F, 64) + _cdiv(3 * n_loc, 4 * g) + _cdiv(g, 256) + 14 + 4


def depth_fused(F, n_loc):
    nb = _cdiv(3 * n_loc, 32)
    return 4 * _cdiv(F, 32) + _cdiv(nb, 1024) + 12 + 20


def depth_e0(F):
    return 3 * _cdiv(pad16(F), 128) + 7


def depth_rowsum(F):
    return _cdiv(pad16(F), 128) + 7


def depth_totals(n_loc, cap):
    g = energy_grid(n_loc, cap)
    return _cdiv(n_loc, 4 * g) + _cdiv(g, 256) + 10


def depth_stream(T, E2):
    return 3 * E2 + 7 + T // 64


def depth_moments(n_loc):
    return _cdiv(n_loc, 1024) + 6 + 16


def sum_bound(depth, abs_sum, extra=0):
    """(depth + 2 + extra) u sum |term|, as a float"""
    return float((depth + 2 + extra) * U * LD(abs_sum))


def energy_bounds(en):
    """en = ld_energies(T) -> (bound of E0, bound of m_v, bound of EV), per vertex, longdouble"""
    F = en["F"]
    bE0 = (depth_e0(F) + 2 + 1) * U * en["E0"]
    ds = (depth_rowsum(F) + 2) * U * en["A"]
    bmv = ((2 * np.abs(en["s"]) * ds + ds * ds).sum(axis=1) + 6 * U * (en["s"] ** 2).sum(axis=1)) / LD(F)
    bEV = bE0 + bmv + U * np.maximum(en["E0"], en["mv"])
    return bE0, bmv, bEV


def quotient_bound(num, den, bnum, bden):
    """|d(num / den)| <= (bnum + |num / den| bden) / |den| + u |num / den| (first order, one rounding of the quotient)"""
    q = abs(LD(num) / LD(den))
    return float((LD(bnum) + q * LD(bden)) / abs(LD(den)) + U * q)


def cv2_bound(n, S1, S2, b1, b2):
    """ev_cv2 = n S2 / S1^2 - 1: first-order propagation plus four host roundings of n S2 / S1^2"""
    S1, S2 = LD(S1), LD(S2)
    r = LD(n) * S2 / (S1 * S1)
    return float(LD(n) * LD(b2) / (S1 * S1) + 2 * r * LD(b1) / S1 + 4 * U * r + U * abs(r - 1))


def psf_rel_bound(var_rel_bound):
    """1 / sqrt(var): half the relative bound of var, the sqrt and the division"""
    return 0.5 * float(var_rel_bound) + 2 * U + float(var_rel_bound) ** 2


def var_rel_bound(sums, mu_true, var_true, depth_sum, depth_sq, one_sweep, world=1):
    """relative bound of the var standarize() forms, from the longdouble sums of the tensor it was formed on.
    two passes: sqdev's own bound (three roundings per term) + count dmu^2 + the division;
    one sweep: the errors of S2 / count and of mu^2 through S1, plus 2 u (1 + mu^2 / var)."""
    n = LD(sums["count"])
    var = LD(var_true)
    dmu = (LD(sum_bound(depth_sum + world, sums["abs"])) / n) + U * abs(LD(mu_true))
    if not one_sweep:
        b = LD(sum_bound(depth_sq + world, var * n, extra=3)) / n + dmu * dmu + U * var
        return float(b / var)
    b2 = LD(sum_bound(depth_sq + world, sums["sq"], extra=1)) / n
    b = b2 + 2 * abs(LD(mu_true)) * dmu + dmu * dmu
    return float(b / var + 2 * U * (1 + LD(mu_true) ** 2 / var))
