"""Shared by tests/test_pins_cpu.py, tests/test_gpu_pins.py and tools/gen_golden_pins.py: positional constraints (pins) on top of
the NumPy f64 model of tests/pdsolve_cases.py / tests/rollout_cases.py, and the bound a pinned result is held to.

The reference's ``PositionalConstraint`` (Constraint_projections.py:77-113) holds vertex v_i at p0_i + shift[row] with weight wi_i:
wi_i joins A at (v_i, v_i) and wi_i (p0_i + shift[row]) joins b at v_i (``project_to_positional_constraint_manifold``,
Simulators.py:401-413, the first summand of :513-520).  ``row`` is the reference's step counter ``self.frame``: f when it steps
from the state of frame f, one more per further step.  The term does not depend on q, so the model adds it to the constant of
a step: const = M / dt^2 s + pin term, b = sum of the kinds + const.

The fixtures (tests/golden/pins_<name>.npz, tools/gen_golden_pins.py) take the element sets and frames of the cproj fixtures:

    edge_spring_fixed   edge springs, pins on vertices 0 and 17, weights 0.7 (the fixtures' WI) and 1e3 (stiff), fixed
    combined_moving     edge springs + tets_strain, pins on vertices 2, 9 and 15, weights 0.7, 1e3 and 1.4, a (T_s, P, 3) shift

both explicit states, gravity ``G`` on, K in {1, 3, 10}, start frames range(0, 130, 3), T = 1 and the steps of
``rollout_cases.STEPS`` -- those whose amplification, measured ON THIS MODEL as ``rollout_cases.measure_amp`` measures it
(``measure_amp`` below: the same draws, with the pin term and gravity), stays <= ``pdsolve_cases.AMP_CAP`` = 1e3.

Bound.  B = 2 max(1, amp_T) T (K one + adv) of rollout_cases, with the one-iteration bound of gstep_cases extended by the pin
term: the device forms t = fl(p0 + shift), term = fl(wi t), const = fl(ms + term) -- three roundings of numbers no larger than
max(wi |target|) (ms's own rounding is in the force bound's companion 64 eps kappa max |q|), passed through A^-1:

    one = || |A^-1| ||_inf (force bound + 3 eps max(wi |target|)) + 64 eps kappa(A) max |q|

with A the matrix that holds the pins' weights.  Nothing here is fitted to the code under test."""
import numpy as np
from scipy import sparse
from scipy.sparse.linalg import splu

import pdsolve_cases as pc
import rollout_cases as rc
from pdsolve_cases import AMP_CAP, KS, MODES      # noqa: F401
from rollout_cases import EPS, START_FRAMES      # noqa: F401

G = (0.0, -9.81, 0.3)
T_S = 140                   # rows of the moving fixture's shift: start frame 129 and 8 steps read row 136
WI = 0.7
FIXTURES = {
    "edge_spring_fixed": dict(base="edge_spring", vertices=(0, 17), wi=(0.7, 1e3), moving=False),
    "combined_moving": dict(base="combined", vertices=(2, 9, 15), wi=(0.7, 1e3, 1.4), moving=True),
}
_cache = {}


def steps_of(name):
    """T = 1 (``solve_frames``) and the roll-out lengths of the fixture's element set."""
    return (1,) + tuple(rc.STEPS[FIXTURES[name]["base"]])


def shift_of(P, rows=T_S):
    """A smooth per-pin path (rows, P, 3), a few percent of the meshes' size, every row different."""
    r = np.arange(rows, dtype=np.float64)[:, None, None]
    i = np.arange(P, dtype=np.float64)[None, :, None]
    d = np.arange(3, dtype=np.float64)[None, None, :]
    return 0.04 * np.sin(0.13 * r + 0.9 * i + 0.5 * d) + 0.0007 * r * (d - 1.0)


def pins_of(name, rest):
    """The ``pins=`` dict of the public interface for a fixture; ``rest`` (N, 3): the reference's ``positions`` (p0 = rest[v])."""
    f = FIXTURES[name]
    v = np.array(f["vertices"], dtype=np.int64)
    out = dict(vertices=v, wi=np.array(f["wi"]), positions=np.array(rest)[v])
    if f["moving"]:
        out["shift"] = shift_of(v.size)
    return out


def with_pins(c, pins):
    """A copy of a case of ``pdsolve_cases.host_case`` (or one shaped like it, with ``wi`` per kind in ``c['wis']`` or the
    fixtures' 0.7) whose matrix holds the pins' weights, plus ``pins`` = (vertices, wi (P,), p0 (P, 3), shift or None)."""
    from animsnapbases_amd import projections as proj
    v = np.asarray(pins["vertices"], dtype=np.int64)
    w = np.broadcast_to(np.asarray(pins["wi"], dtype=np.float64), v.shape).copy()
    N = c["masses"].shape[0]
    wis = c.get("wis", [WI] * len(c["kinds"]))
    A = proj.global_matrix([(k[0], wk) for k, wk in zip(c["kinds"], wis)], N, c["masses"], c["dt"], (v, w))
    shift = pins.get("shift")
    shift = None if shift is None else np.asarray(shift, dtype=np.float64)
    if shift is not None and shift.ndim == 2:
        shift = np.repeat(shift[:, None, :], v.size, axis=1)
    return dict(c, A=A, lu=splu(sparse.csc_matrix(A)), pins=(v, w, np.asarray(pins["positions"], dtype=np.float64), shift))


def host_case(name, load=pc._load):
    """The host case of a fixture: the element set's case of ``pdsolve_cases`` with the pins in A.  Built once."""
    if name not in _cache:
        base = pc.host_case(FIXTURES[name]["base"], load)
        rest = load("cproj_" + pc.parts_of(FIXTURES[name]["base"])[-1])["rest"]
        _cache[name] = with_pins(base, pins_of(name, rest))
    return _cache[name]


def targets(c, rows):
    """(F', P, 3): p0 + shift[row] per frame, in the engine's order (one rounding)."""
    v, w, p0, shift = c["pins"]
    rows = np.asarray(rows, dtype=np.int64)
    return np.broadcast_to(p0[None], (rows.size,) + p0.shape) if shift is None else p0[None] + shift[rows]


def pin_term(c, rows):
    """(F', N, 3): wi (p0 + shift[row]) at the pinned vertices, +0.0 elsewhere."""
    v, w = c["pins"][:2]
    out = np.zeros((len(rows), c["masses"].shape[0], 3))
    out[:, v] = w[None, :, None] * targets(c, rows)
    return out


def iterate(c, s, q, K, rows, reduced=None):
    """``rollout_cases.iterate`` with the pin term of the rows ``rows`` (one per frame) in the constant."""
    from animsnapbases_amd import projections as proj
    const = (c["masses"] / c["dt"] ** 2)[None, :, None] * s + pin_term(c, rows)
    for _ in range(K):
        b = None
        for i, (setup, St, smin, smax) in enumerate(c["kinds"]):
            if reduced is not None and reduced[0] == i:
                term = pc.reduced_term(setup, St, reduced[1], q, smin, smax)
            else:
                p = proj.project_host(setup, q, smin, smax)
                term = np.stack([St @ p[f] for f in range(q.shape[0])])
            b = term if b is None else b + term
        b = b + const
        q = np.stack([c["lu"].solve(b[f]) for f in range(q.shape[0])])
    return q


def rollout(c, K, T, s, p, rows, acc=None, reduced=None, first=None):
    """[q_1, .., q_T] as ``rollout_cases.rollout``; step t reads the rows ``rows`` + t - 1."""
    rows = np.asarray(rows, dtype=np.int64)
    out = []
    for t in range(T):
        q = iterate(c, s, s if first is None or t else first, K, rows + t, reduced)
        out.append(q)
        s, p = rc.carry(q, p, acc)
    return out


def measure_amp(c, mode, K, T, sel=START_FRAMES, acc=None, reduced=None, seed=0):
    """``rollout_cases.measure_amp`` on the pinned model: the same sizes, draws and seed, gravity and the pin term included."""
    frames, sel = c["frames"], list(sel)
    prev = [max(f - 1, 0) for f in sel]
    x, xp = frames[sel], frames[prev]
    a = 0.0 if acc is None else np.asarray(acc)[None, None, :]
    make = lambda x, xp: ((x if mode == "zero" else 2.0 * x - xp) + a, x)
    base = rollout(c, K, T, *make(x, xp), sel, acc, reduced)
    rng = np.random.default_rng(seed)
    amp = np.zeros(T)
    for size in (1e-9, 1e-12):
        for _ in range(3):
            s, p = make(x + size * rng.standard_normal(x.shape), xp + size * rng.standard_normal(x.shape))
            runs = [rollout(c, K, T, s, p, sel, acc, reduced)]
            s, p = make(x, xp)
            runs.append(rollout(c, K, T, s, p, sel, acc, reduced, first=s + size * rng.standard_normal(x.shape)))
            for got in runs:
                for t in range(T):
                    amp[t] = max(amp[t], float(np.abs(got[t] - base[t]).max() / size))
    return np.maximum.accumulate(amp)


def matrix_numbers(c):
    """(|| |A^-1| ||_inf, kappa(A)) of the case's matrix, pins included."""
    Ad = c["A"].toarray()
    return float(np.abs(np.linalg.inv(Ad)).sum(axis=1).max()), float(np.linalg.cond(Ad))


def pin_rounding(c, rows):
    """3 eps max(wi |target|): the three roundings of the pin term (module docstring), before A^-1."""
    return 3.0 * EPS * float(np.abs(pin_term(c, rows)).max())


def one_bound(c, force_bound, q_max, rows):
    """The one-iteration bound of the module docstring as one number."""
    ainv, kappa = matrix_numbers(c)
    return ainv * (float(np.max(force_bound)) + pin_rounding(c, rows)) + 64.0 * EPS * kappa * float(q_max)
