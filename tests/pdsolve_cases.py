"""Shared by tests/test_pdsolve_cpu.py, tests/test_gpu_pdsolve.py and tools/gen_golden_pdsolve.py: a NumPy f64 model of the
solver's loop (Simulators.py:506-526) built from ``projections.project_host``, ``assembly_ST``, ``global_matrix``, SciPy's
``splu`` and ``reduced.reduced_operator`` -- also the host route of the reduced solve -- and the bound a K-iteration result
is held to.

One iteration is held to the bound of tests/gstep_cases.py (``step_bound``; for a reduced kind || |A^-1| ||_inf times the
bound of tests/reduced_forces_cases.py takes the place of the force bound).  An error made in an earlier iteration passes
through the remaining ones.  The projections are not globally Lipschitz (determinant flips), so that amplification cannot be
derived; it is MEASURED ON THIS MODEL, never on the code under test: the start is perturbed by Gaussian noise of size 1e-9
and 1e-12 (three draws each), K iterations are run and the largest max |dq_K| / size over all frames and draws is ``amp``
(tools/gen_golden_pdsolve.py stores it per fixture, mode and K).  K iterations commit K one-iteration errors, each amplified
by at most max(1, amp); sampled perturbations under-estimate a supremum, hence the factor 2:

    B_K = 2 K max(1, amp) (one-iteration bound)

A fixture whose amp exceeds 1e3 for some frame is unsuitable and is to be changed; no frame is ever left out."""
import numpy as np
from scipy import sparse
from scipy.sparse.linalg import splu

KS = (1, 3, 10)
MODES = ("zero", "difference")
NAMES = ["edge_spring", "tris_strain", "tets_strain", "tets_deformation_gradient", "combined"]
AMP_CAP = 1e3
_cache = {}


def _load(name):
    from conftest import load_golden
    return load_golden(name)


def parts_of(name):
    """The cproj fixtures of a pdsolve fixture, in the solver's order; the frames are those of the last."""
    return ["edge_spring", "tets_strain"] if name == "combined" else [name]


def host_case(name, load=_load, wi=0.7):
    """frames, rest, per kind (setup, S^T, sigma_min, sigma_max), A (CSR), masses, dt of a pdsolve fixture, from the cproj and
    gstep fixtures and the package's own host routines.  Read once, read-only."""
    if name not in _cache:
        from animsnapbases_amd import projections as proj
        gs = [load("cproj_" + k) for k in parts_of(name)]
        z = load("gstep_" + name)
        N = gs[-1]["rest"].shape[0]
        kinds = []
        for k, g in zip(parts_of(name), gs):
            setup = proj.build_setup(k, g["elements"], g["rest"])
            kinds.append((setup, proj.assembly_ST(setup, N, wi), float(g["sigma"][0]), float(g["sigma"][1])))
        masses, dt = np.array(z["masses"]), float(z["dt"])
        A = proj.global_matrix([(q[0], wi) for q in kinds], N, masses, dt)
        frames = np.array(gs[-1]["frames"])
        frames.setflags(write=False)
        _cache[name] = dict(name=name, frames=frames, kinds=kinds, A=A, masses=masses, dt=dt, lu=splu(sparse.csc_matrix(A)))
    return _cache[name]


def explicit_state(frames, sel, mode, acc=None):
    """s_f of the selected frames: x_f (+ acc) or 2 x_f - x_{f-1} (+ acc), f - 1 the animation's previous frame (x_0 at 0)."""
    sel = list(sel)
    x = frames[sel]
    s = x if mode == "zero" else 2.0 * x - frames[[max(f - 1, 0) for f in sel]]
    return s if acc is None else s + np.asarray(acc)[None, None, :]


def reduced_term(setup, St, op, q, smin, smax):
    """b~ = S^T V (P^T V)^+ P^T p(q) per coordinate (the host projects every element and keeps the sampled rows Pt)."""
    from animsnapbases_amd import projections as proj
    P = proj.project_host(setup, q, smin, smax)[:, op.Pt]
    out = np.empty(q.shape)
    for d in range(3):
        out[:, :, d] = ((St @ op.V[:, :, d]) @ (op.H[d] @ P[:, :, d].T)).T
    return out


def model(c, sel, mode, Ks, start="explicit", acc=None, reduced=None):
    """{K: q after K iterations, (F', N, 3)} for the frames ``sel`` of case ``c``.  ``start``: "explicit", "frame" or an array;
    ``reduced``: None or (index of the kind, ``reduced.ReducedOperator``)."""
    from animsnapbases_amd import projections as proj
    frames, sel = c["frames"], list(sel)
    s = explicit_state(frames, sel, mode, acc)
    ms = (c["masses"] / c["dt"] ** 2)[None, :, None] * s
    q = s.copy() if isinstance(start, str) and start == "explicit" else (frames[sel].copy() if isinstance(start, str) else np.array(start))
    out = {0: q.copy()} if 0 in Ks else {}
    for k in range(1, max(Ks) + 1):
        b = None
        for i, (setup, St, smin, smax) in enumerate(c["kinds"]):
            if reduced is not None and reduced[0] == i:
                term = reduced_term(setup, St, reduced[1], q, smin, smax)
            else:
                p = proj.project_host(setup, q, smin, smax)
                term = np.stack([St @ p[f] for f in range(len(sel))])
            b = term if b is None else b + term
        b = b + ms
        q = np.stack([c["lu"].solve(b[f]) for f in range(len(sel))])
        if k in Ks:
            out[k] = q.copy()
    return out


def measure_amp(c, mode, Ks=KS, reduced=None, seed=0):
    """{K: the largest max |dq_K| / size over all frames and draws} (module docstring)."""
    sel = range(c["frames"].shape[0])
    s = explicit_state(c["frames"], sel, mode)
    base = model(c, sel, mode, Ks, reduced=reduced)
    rng = np.random.default_rng(seed)
    amp = {K: 0.0 for K in Ks}
    for size in (1e-9, 1e-12):
        for _ in range(3):
            got = model(c, sel, mode, Ks, start=s + size * rng.standard_normal(s.shape), reduced=reduced)
            for K in Ks:
                amp[K] = max(amp[K], float(np.abs(got[K] - base[K]).max() / size))
    return amp


def bound_K(one, K, amp):
    assert amp <= AMP_CAP, "amp %.3g: the fixture is unsuitable (change it; no frame is left out)" % amp
    return 2.0 * K * max(1.0, float(amp)) * one


def chain(n, seed=0):
    """An edge-spring chain of n vertices along a wavy line: rest (n, 3), edges (n - 1, 2), masses (n,)."""
    rng = np.random.default_rng(1000 + n + seed)
    rest = np.stack([0.4 * np.arange(n), 0.1 * np.sin(0.9 * np.arange(n)), 0.05 * rng.standard_normal(n)], axis=1)
    edges = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1).astype(np.int64)
    return rest, edges, 0.5 + rng.random(n)


def animate(rest, F, seed=0, amp=0.03):
    """F frames around ``rest``: a smooth sway plus small noise, every frame different."""
    rng = np.random.default_rng(seed)
    t = np.arange(F)[:, None, None]
    phase = rng.uniform(0, 2 * np.pi, size=(1, rest.shape[0], 3))
    return rest[None] * (1.0 + 0.05 * np.sin(0.21 * t)) + amp * np.sin(0.37 * t + phase) + 0.002 * rng.standard_normal((F,) + rest.shape)
