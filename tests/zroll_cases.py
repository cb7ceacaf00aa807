"""Shared by tests/test_zroll_cpu.py and tests/test_gpu_zroll.py: the cases of the roll-outs whose state lives in z
and the bounds the device's results are held to.  Nothing is fitted to the code under test; every term is derived here, for the
error in q = o + U z (an error e_z in z is the error |U| e_z in q).

ONE ITERATION of a step, z' = c_z + sum_k G_k coef_k, c_z = kappa + T y + E target, then q' = o_t + U_t z' (``one_bound``):
  chains    an entry of z' is two chains of MFMAs, of length r + P (c_z) and sum_k m_k (the update), each from a zero accumulator
            and rounded once more when its base is added: (sum m_k + r + P + 16) eps times the sum of the absolute values of its
            terms, S_z = |kappa| + |T| |y| + |E| |target| + sum_k |G_k| |coef_k|, passed through |U|.  The touched expansion is a
            chain of length r: (r + 2) eps (|o| + |U| |z'|).
  once      T, kappa, E and G_k are each W R for a handful of columns R (D U, D (o + a) - A o, w_i e_{v_i}, S_k^T V_k), formed
            once per call by the reduce of asb_gsub.hip -- a chain of length N per entry -- with W = fl(U At^-1)^T.  Multiplied out,
            U z' = U W (D U y + D (o + a) - A o + pins + sum_k M_k coef_k): the linear map of ``gsub_cases.apply_bound`` on the
            right-hand side of the Galerkin step, term by term.  Chains: (N + 2 r + 16) eps max of |U| (|At^-1| (|U^T| R_abs)) with
            R_abs the sum of the terms' absolute values; inverse: 64 eps kappa(At_d) times the sum over the terms of
            max |U| |W R_term| (the form of DESIGN.md 3.13, as ``gsub_cases.hyper_bound`` sums it).  A o itself is a sparse
            product, (row entries + 2) eps |A| |o| through |U| |At^-1| |U^T|; D (o + a) rounds twice: 2 eps of its size, inside R_abs's
            factor 16.
  coef      || |P| ||_inf (``gsub_cases.p_abs_inf``) times ``hyper_cases.reduced_force_bound`` of every kind (N more terms in its
            dot products: M is formed by a sparse product and G by the chain over N), at the projections of the iterate, with
            kappa_d = 0 (``conds_of``: the model multiplies by the device's own H_d).
  pins      target = fl(p0 + shift) and the product with w_i inside E: ``pins_cases.pin_rounding`` (3 eps max w |target|)
            through || |P| ||_inf.

THE CARRY y = fl(2 z - z_p) rounds once, 2 z being exact; ``adv_bound`` takes 2 eps (2 |z| + |z_p|) through |U|.

THE START z_0 = U^T (x_f - o), z_-1 likewise: a chain of length N and the subtraction, (N + 2) eps |U^T| |x - o| per entry of z,
through |U| in q (``start_bound``; y = 2 z_0 - z_-1 carries three of them).  It is a perturbation of the state, so it is amplified
like every other error.

K ITERATIONS AND T STEPS: ``rollout_cases.bound_T(one, K, T, amp, adv)`` = 2 max(1, amp) T (K one + adv), plus 2 max(1, amp)
start, with amp MEASURED ON THE HOST MODEL, never on the code under test: ``rollout_cases.measure_amp`` /
``pins_cases.measure_amp`` on the case whose ``lu`` is the Galerkin map and whose frames are projected into o + span(U); for two
reduced kinds ``measure_amp_multi``, the same sizes, draws and seed on the same loop with a dict of operators.
Condition: amp <= AMP_CAP = 1000 (``bound_T`` asserts it); tests/test_zroll_cpu.py measures exactly the combinations that run.

The cases.  ``tris_blocks`` (N = 42): r in {4, 8}, m in {3, 8}, K in {1, 3}, T = 5.  ``tets_deim`` (N = 18), m = 17, unpinned:
(r, K, T) in ``TETS_ROWS`` = (4, 1, 5), (4, 3, 5), (8, 1, 2), (8, 3, 2) and no others ((8, 3, 5) measures amp 8.4e3, above the
cap).  Pins on both: fixed (vertices 0, 17; w 0.7, 1e3) and moving (2, 9, 15; w 0.7, 1e3, 1.4; ``pins_cases.shift_of``), gravity
``pins_cases.G``, r = 4, the largest m, K = 3, T = 5.  Start frames ``rollout_cases.START_FRAMES``, both velocity modes."""
import numpy as np

import gsub_cases as gc
import pdsolve_cases as pc
import pins_cases as pins
import reduced_forces_cases as rf
import rollout_cases as rc
from gsub_model import EPS, LD, vertex_major
from hyper_cases import reduced_force_bound
from pdsolve_cases import AMP_CAP, MODES      # noqa: F401
from zroll_model import ZModel

RAW_TOL = rf.RAW_TOL
SEL = rc.START_FRAMES
TRIS_ROWS = [(r, m, K, 5) for r in (4, 8) for m in (3, 8) for K in (1, 3)]
TETS_ROWS = [(4, 17, 1, 5), (4, 17, 3, 5), (8, 17, 1, 2), (8, 17, 3, 2)]
FREE = [("tris_blocks",) + row for row in TRIS_ROWS] + [("tets_deim",) + row for row in TETS_ROWS]
PIN_SETS = {"fixed": dict(vertices=(0, 17), wi=(0.7, 1e3), moving=False), "moving": dict(vertices=(2, 9, 15), wi=(0.7, 1e3, 1.4), moving=True)}
PINNED = [(fx, pn, 4, m, 3, 5) for fx, m in (("tris_blocks", 8), ("tets_deim", 17)) for pn in ("fixed", "moving")]
_cache = {}


def pins_dict(pn, rest):
    f = PIN_SETS[pn]
    v = np.array(f["vertices"], dtype=np.int64)
    out = dict(vertices=v, wi=np.array(f["wi"]), positions=np.array(rest)[v])
    if f["moving"]:
        out["shift"] = pins.shift_of(v.size)
    return out


def z_case(fixture, r, pn=None):
    """The subspace case of a reduced-forces fixture: ``gsub_cases.sub_case`` of its kind (with the pins ``pn`` in the matrix), plus
    ``rf`` (the fixture), ``pins_dict`` and ``proj_frames``: the frames projected into o + span(U), read-only."""
    key = (fixture, r, pn)
    if key not in _cache:
        c = rf.case(fixture)
        base = pc.host_case(c.kind)
        pd = None
        if pn is not None:
            pd = pins_dict(pn, c.g["rest"])
            base = pins.with_pins(base, pd)
        s = dict(gc.sub_case(c.kind, r, base=base), rf=c, pins_dict=pd)
        g = s["galerkin"]
        x = np.asarray(s["frames"], dtype=np.float64).astype(LD)
        pf = np.stack([g.o[None, :, d] + ((x[:, :, d] - g.o[None, :, d]) @ g.U[d]) @ g.U[d].T for d in range(3)], axis=2).astype(np.float64)
        pf.setflags(write=False)
        s["proj_frames"] = pf
        _cache[key] = s
    return _cache[key]


def operator(s, m):
    return rf.operator(s["rf"], m)


def amp_of(s, m, mode, K, T, acc=None):
    """(T,) the amplification of the host model under the subspace on the projected frames (module docstring), cached."""
    key = ("amp", s["rf"].name, s["r"], s["pins_dict"] is not None and tuple(s["pins_dict"]["vertices"]), m, mode, K, T, acc is not None)
    if key not in _cache:
        c = dict(s, frames=s["proj_frames"])
        red = (0, operator(s, m))
        if s["pins_dict"] is None:
            assert acc is None
            _cache[key] = rc.measure_amp(c, mode, K, T, SEL, reduced=red)
        else:
            _cache[key] = pins.measure_amp(c, mode, K, T, SEL, acc, reduced=red)
    return _cache[key]


def _iterate_multi(c, s, q, K, ops):
    """``rollout_cases.iterate`` with a dict of reduced kinds (every kind of the case)."""
    ms = (c["masses"] / c["dt"] ** 2)[None, :, None] * s
    for _ in range(K):
        b = None
        for i, (setup, St, smin, smax) in enumerate(c["kinds"]):
            term = pc.reduced_term(setup, St, ops[i], q, smin, smax)
            b = term if b is None else b + term
        b = b + ms
        q = np.stack([c["lu"].solve(b[f]) for f in range(q.shape[0])])
    return q


def _rollout_multi(c, K, T, s, p, ops, first=None):
    out = []
    for t in range(T):
        q = _iterate_multi(c, s, s if first is None or t else first, K, ops)
        out.append(q)
        s, p = rc.carry(q, p)
    return out


def measure_amp_multi(c, mode, K, T, ops, sel=SEL, seed=0):
    """``rollout_cases.measure_amp`` -- the same sizes, draws and seed -- for a case with several reduced kinds."""
    frames, sel = c["frames"], list(sel)
    x, xp = frames[sel], frames[[max(f - 1, 0) for f in sel]]
    make = lambda x, xp: (x.copy() if mode == "zero" else 2.0 * x - xp, x)
    base = _rollout_multi(c, K, T, *make(x, xp), ops)
    rng = np.random.default_rng(seed)
    amp = np.zeros(T)
    for size in (1e-9, 1e-12):
        for _ in range(3):
            s, p = make(x + size * rng.standard_normal(x.shape), xp + size * rng.standard_normal(x.shape))
            runs = [_rollout_multi(c, K, T, s, p, ops)]
            s, p = make(x, xp)
            runs.append(_rollout_multi(c, K, T, s, p, ops, first=s + size * rng.standard_normal(x.shape)))
            for got in runs:
                for t in range(T):
                    amp[t] = max(amp[t], float(np.abs(got[t] - base[t]).max() / size))
    return np.maximum.accumulate(amp)


# ------------------------------------------------------------------ the bounds
def _abs64(x):
    return np.abs(x).astype(np.float64)


def _through_U(zm, ez):
    """max over the coordinates of |U_d| e_z for e_z (F, r, 3) >= 0."""
    return max(float((ez[:, :, d] @ _abs64(zm.g.U[d]).T).max()) for d in range(3))


def start_bound(zm, x):
    """One projection z = U^T (x - o) of the frames x (F, N, 3), as an error in q."""
    g = zm.g
    return max(float(((g.N + 2) * EPS * (np.abs(x[:, :, d] - g.o[None, :, d].astype(np.float64)) @ _abs64(g.U[d])) @ _abs64(g.U[d]).T).max())
               for d in range(3))


def adv_bound(zm, rec):
    return _through_U(zm, 2.0 * EPS * (2.0 * np.abs(rec["z_in"]) + np.abs(rec["zp"])))


def one_bound(zm, rec, conds, tol_p=RAW_TOL):
    """The bound of one iteration (module docstring), the largest over the iterations of the step recorded in ``rec``;
    ``conds``: {index of a kind: the (3,) condition numbers of its normal matrices}."""
    g, s = zm.g, zm.s
    N, r = g.N, g.r
    P = 0 if zm.pins is None else len(zm.pins[0])
    msum = sum(op.H.shape[1] for op in zm.ops.values())
    pinf = gc.p_abs_inf(g)
    A64, o64 = _abs64(g.A), _abs64(g.o)
    row = int((A64 != 0).sum(axis=1).max())
    sparse_err = (row + 2) * EPS * float(g.magnitude(vertex_major((A64 @ o64)[None])).max())
    D = zm.D.astype(np.float64)
    y, tgt = rec["y"], rec["tgt"]
    F = y.shape[0]
    pin_round = 0.0
    if tgt is not None:
        pin_round = 3.0 * EPS * float((zm.pins[1][None, :, None] * np.abs(tgt)).max())
    worst = 0.0
    for it in rec["its"]:
        per_d = []
        for d in range(3):
            U, W = g.U[d], g.W[d]
            aU = _abs64(U)
            Sz = _abs64(zm.kappa[d])[None, :] + np.abs(y[:, :, d]) @ _abs64(zm.T[d]).T
            terms = [(D[:, None] * U.astype(np.float64)) @ y[:, :, d].T, np.repeat(zm.const[d].astype(np.float64)[:, None], F, axis=1)]
            Rabs = (D[:, None] * aU) @ np.abs(y[:, :, d]).T + (D * (o64[:, d] + abs(float(zm.a[d]))) + _abs64(g.Ao[:, d]))[:, None]
            if tgt is not None:
                Sz = Sz + np.abs(tgt[:, :, d]) @ _abs64(zm.E[d]).T
                pt = np.zeros((N, F))
                pt[zm.pins[0]] = (zm.pins[1][None, :] * tgt[:, :, d]).T
                terms.append(pt)
                Rabs = Rabs + np.abs(pt)
            for i in sorted(zm.ops):
                co = it["coef"][i][d]
                Sz = Sz + np.abs(co).T @ _abs64(zm.G[i][d]).T
                terms.append(zm.M[i][d].astype(np.float64) @ co)
                Rabs = Rabs + _abs64(zm.M[i][d]) @ np.abs(co)
            chains = (msum + r + P + 16) * EPS * float((Sz @ aU.T).max())
            expand = (r + 2) * EPS * float((o64[None, :, d] + np.abs(it["z"][:, :, d]) @ aU.T).max())
            once_chain = (N + 2 * r + 16) * EPS * float((aU @ (_abs64(g.Ai[d]) @ (aU.T @ Rabs))).max())
            once_inv = 64 * EPS * g.kappa[d] * sum(float((aU @ _abs64(W @ t.astype(LD))).max()) for t in terms)
            per_d.append(chains + expand + once_chain + once_inv)
        red = sum(float(reduced_force_bound(s["kinds"][i][1], zm.ops[i], it["P"][i], conds[i], tol_p, N).max()) for i in zm.ops)
        worst = max(worst, max(per_d) + pinf * (red + pin_round) + sparse_err)
    return worst


def bounds(zm, recs, K, amp, conds, start):
    """[B_t for t = 1 .. T]: ``rollout_cases.bound_T`` with the largest one-iteration and carry bounds of the steps so far, plus
    the amplified start error (``start``: the sum of the start's projection roundings in q; 0 for a given state)."""
    out, one, adv = [], 0.0, 0.0
    for t, rec in enumerate(recs):
        one, adv = max(one, one_bound(zm, rec, conds)), max(adv, adv_bound(zm, rec))
        a = float(amp[t])
        out.append(rc.bound_T(one, K, t + 1, a, adv) + 2.0 * max(1.0, a) * start)
    return out


def conds_of(ops):
    """The condition numbers ``reduced_force_bound`` takes: zero.  kappa_d is in that bound because ITS reference solves the
    normal equations (A^T A + la I) x = A^T p by LU while the device multiplies by the explicit H_d; ``ZModel.coefficients``
    multiplies by the very H_d the device is given, so that difference does not exist here.  What remains of the first term are
    the lengths of the dot products (mp + |Pt| + N)."""
    return {i: np.zeros(3) for i in ops}
