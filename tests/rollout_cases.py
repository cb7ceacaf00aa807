"""Shared by tests/test_rollout_cpu.py, tests/test_gpu_rollout.py and tools/gen_golden_rollout.py: a NumPy f64 model of the
reference's time steps (Simulators.py ``step()``: the loop :506-526, then :531-532 velocities = (q - positions) / dt,
positions = q, and the next explicit state :495) built on tests/pdsolve_cases.py, and the bound a T-step result is held to.

A step is K iterations from q_0 = s_t followed by the carry s_{t+1} = 2 q - p_t + acc, p_{t+1} = q.  One iteration is held to
the one-iteration bound of pdsolve_cases / gstep_cases (``one``).  The carry rounds twice, fl(fl(2 q - p) + acc) (2 q is
exact), so it commits at most

    adv = 2 eps (2 |q| + |p| + |acc|)

per entry (``adv_bound``; the reference's own q + dt ((q - p) / dt) rounds twice too when dt is a power of two, as the
fixtures' dt = 0.5 is).  T steps commit T (K one + adv); an error made early passes through the remaining iterations AND
steps.  That amplification cannot be derived (determinant flips; the carry doubles a perturbation of q), so it is MEASURED ON
THIS MODEL, never on the code under test (``measure_amp``): Gaussian perturbations of size 1e-9 and 1e-12, three draws each,
of (a) the state (x_f, x_{f-1}) and (b) the first iterate alone; amp_T is the largest max |dq_t| / size over all start frames,
draws and steps t <= T.  Sampled perturbations under-estimate a supremum, hence the factor 2 of pdsolve_cases:

    B = 2 max(1, amp_T) T (K one + adv)

Condition: amp_T <= AMP_CAP = 1e3 (pdsolve_cases).  tools/gen_golden_rollout.py asserts it and stores amp_T with the fixtures;
no start frame is left out of any comparison.  ``tets_strain`` and ``combined`` leave the cap from step 3-4 on (inverted
elements flip), so their fixtures stop at T = 2; the three smooth ones go to T = 8."""
import numpy as np

from pdsolve_cases import AMP_CAP, KS, MODES, NAMES, explicit_state, reduced_term      # noqa: F401

EPS = np.finfo(np.float64).eps
START_FRAMES = list(range(0, 130, 3))
LONG = (2, 5, 8)
STEPS = {"edge_spring": LONG, "tris_strain": LONG, "tets_deformation_gradient": LONG, "tets_strain": (2,), "combined": (2,)}
REDUCED = {"tets_deim": "tets_strain", "tris_blocks": "tris_strain"}


def iterate(c, s, q, K, reduced=None):
    """K iterations of the solver's loop from ``q`` with the explicit state ``s`` (both (F', N, 3)) for the case ``c`` of
    ``pdsolve_cases.host_case``; ``reduced``: None or (index of the kind, ``reduced.ReducedOperator``)."""
    from animsnapbases_amd import projections as proj
    ms = (c["masses"] / c["dt"] ** 2)[None, :, None] * s
    for _ in range(K):
        b = None
        for i, (setup, St, smin, smax) in enumerate(c["kinds"]):
            if reduced is not None and reduced[0] == i:
                term = reduced_term(setup, St, reduced[1], q, smin, smax)
            else:
                p = proj.project_host(setup, q, smin, smax)
                term = np.stack([St @ p[f] for f in range(q.shape[0])])
            b = term if b is None else b + term
        b = b + ms
        q = np.stack([c["lu"].solve(b[f]) for f in range(q.shape[0])])
    return q


def carry(q, p, acc=None):
    """(s_{t+1}, p_{t+1}) of :531-532 and :495 in the engine's order: fl(fl(2 q - p) + acc), q."""
    s = 2.0 * q - p
    return (s if acc is None else s + np.asarray(acc)[None, None, :]), q


def start_state(frames, sel, mode, acc=None):
    """(s_1, p_1) of the selected frames: the explicit state of ``pdsolve_cases.explicit_state`` and x_f."""
    return explicit_state(frames, sel, mode, acc), frames[list(sel)]


def rollout(c, K, T, s, p, acc=None, reduced=None, first=None):
    """[q_1, .., q_T]: T steps of K iterations from the explicit state ``s`` and the positions ``p``; ``first``: the iterate
    the first step starts from in place of s."""
    out = []
    for t in range(T):
        q = iterate(c, s, s if first is None or t else first, K, reduced)
        out.append(q)
        s, p = carry(q, p, acc)
    return out


def measure_amp(c, mode, K, T, sel=START_FRAMES, reduced=None, seed=0):
    """(T,) array: entry t - 1 is the largest max |dq_t'| / size over all frames, draws and steps t' <= t (module docstring)."""
    frames, sel = c["frames"], list(sel)
    prev = [max(f - 1, 0) for f in sel]
    x, xp = frames[sel], frames[prev]
    make = lambda x, xp: (x.copy() if mode == "zero" else 2.0 * x - xp, x)
    base = rollout(c, K, T, *make(x, xp), reduced=reduced)
    rng = np.random.default_rng(seed)
    amp = np.zeros(T)
    for size in (1e-9, 1e-12):
        for _ in range(3):
            s, p = make(x + size * rng.standard_normal(x.shape), xp + size * rng.standard_normal(x.shape))
            runs = [rollout(c, K, T, s, p, reduced=reduced)]
            s, p = make(x, xp)
            runs.append(rollout(c, K, T, s, p, reduced=reduced, first=s + size * rng.standard_normal(x.shape)))
            for got in runs:
                for t in range(T):
                    amp[t] = max(amp[t], float(np.abs(got[t] - base[t]).max() / size))
    return np.maximum.accumulate(amp)


def adv_bound(q, p, acc=None):
    """The rounding of one carry, per module docstring, as one number over the tensors."""
    a = 0.0 if acc is None else float(np.abs(acc).max())
    return 2.0 * EPS * (2.0 * float(np.abs(q).max()) + float(np.abs(p).max()) + a)


def bound_T(one, K, T, amp, adv):
    assert amp <= AMP_CAP, "amp %.3g: the fixture is unsuitable (change it; no frame is left out)" % amp
    return 2.0 * max(1.0, float(amp)) * T * (K * one + adv)
