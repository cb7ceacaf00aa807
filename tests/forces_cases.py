"""Shared by tests/test_forces_cpu.py, tests/test_gpu_forces.py and tools/gen_golden_forces.py: external forces and the floor on top
of the NumPy f64 model of tests/pdsolve_cases.py / tests/rollout_cases.py, and the bound such a result is held to.

The reference's ``step(fext, num_iterations)`` (Simulators.py:480-535) starts with a = fext / mass, explicit = positions +
dt velocities + dt^2 a (:494-495) and ``resolve_collision`` on every vertex of ``explicit`` (:497-498,
Constraint_projections.py:1287-1298: a y below ``floor_height`` is set to it); sn and the first iterate are both the snapped
array.  The model follows the ENGINE's order: gravity stays in acc = dt^2 g, the other forces are the
displacement table fa = dt^2 (force / masses) the host forms, and per entry

    x = fl(fl(fl(2 q - p) + acc) + fa[row]);  if x[axis] < height: x[axis] = height;  s = q_0 = x

with ``row`` the pins' rule: step t = 1, 2, .. from frame f reads row start + f + t - 1.

The fixtures (tests/golden/forces_<name>.npz, tools/gen_golden_forces.py) take the element sets and frames of the cproj fixtures,
the start frames range(0, 130, 3), both explicit states, K in {1, 3, 10}, gravity ``G``, the force ``force_of`` (``T_S`` rows) and

    edge_spring, tris_strain       the floor at the 0.3-quantile of s_1[..., 1] (velocity "zero", gravity in it) over the start frames
    tets_deformation_gradient      no floor: under one its inverted elements flip and the amplification reaches 1e9 - 1e11

The steps ``STEPS`` whose amplification, measured ON THIS MODEL with the table and the floor in the
loop (``measure_amp``: the draws of ``rollout_cases.measure_amp``), stays <= ``pdsolve_cases.AMP_CAP`` = 1e3.

Bound.  B = 2 max(1, amp_T) T (K one + adv) of rollout_cases with adv extended by the one extra rounding of the add,
eps (|x| + |fa|) per entry (``ext_bound``); the clamp is exact and adds none.  Nothing here is fitted to the code under test.

Condition (``check_shares``): in every kept floor case, at every kept step, the reference clamps between 5 % and 95 % of the
(frame, vertex) pairs, and no start frame is left out: a floor that clamps nothing or everything tests nothing."""
import numpy as np

import pdsolve_cases as pc
import rollout_cases as rc
from pdsolve_cases import AMP_CAP, KS, MODES      # noqa: F401
from rollout_cases import EPS, START_FRAMES      # noqa: F401

G = (0.0, -0.3, 0.1)
T_S = 140                   # rows of the force: start frame 129 and 8 steps read row 136
STEPS = (1, 2, 8)           # T = 1 is solve_frames, 2 the first fused advance, 8 the longest of rollout_cases.LONG (the fixture of 42
                            # vertices holds 44 x 42 x 3 doubles per (mode, K, T): a fourth T would pass the size limit of a fixture)
FIXTURES = {"edge_spring": True, "tris_strain": True, "tets_deformation_gradient": False}      # name -> with a floor
SHARE = (0.05, 0.95)


def steps_of(name):
    return STEPS


def force_of(N, rows=T_S, seed=0):
    """(rows, N, 3): the ``force`` of the public interface, 0.2 N(0, 1) -- no row, vertex or coordinate like another."""
    return 0.2 * np.random.default_rng(7000 + N + seed).standard_normal((rows, N, 3))


def fa_of(force, masses, dt):
    """fa = dt^2 (force / masses) in the reference's order (:494-495), as ``dynamics._external`` forms it."""
    return (dt * dt) * (np.asarray(force, dtype=np.float64) / np.asarray(masses)[:, None])


def floor_of(name, frames, acc):
    """The floor height of a fixture, or None."""
    if not FIXTURES[name]:
        return None
    return float(np.quantile(rc.start_state(frames, START_FRAMES, "zero", acc)[0][..., 1], 0.3))


def external(s, fa, floor=None):
    """The engine's two lines on an explicit state ``s`` (F', N, 3): ``fa`` None, (N, 3) or (F', N, 3) (the rows of the frames
    already gathered), ``floor`` None or (height, axis).  Returns (x, clamped (F', N) bool)."""
    x = np.array(s, dtype=np.float64) if fa is None else s + fa
    hit = np.zeros(x.shape[:2], dtype=bool)
    if floor is not None:
        h, axis = floor
        hit = x[..., axis] < h
        x[..., axis] = np.where(hit, h, x[..., axis])
    return x, hit


def rows_of(fa, rows):
    """The table's rows of the frames: ``fa`` None, (N, 3) constant, or (T_s, N, 3) read at ``rows`` (one per frame)."""
    return fa if fa is None or fa.ndim == 2 else fa[np.asarray(rows, dtype=np.int64)]


def rollout(c, K, T, s, p, rows, acc=None, fa=None, floor=None, reduced=None, first=None, shares=None):
    """[q_1, .., q_T] as ``rollout_cases.rollout`` with the force and the floor on every explicit state; step t reads the rows
    ``rows`` + t - 1.  ``first``: a perturbation added to the first iterate alone.  ``shares``: a list that receives the clamped
    share of every step."""
    rows = np.asarray(rows, dtype=np.int64)
    out = []
    for t in range(T):
        x, hit = external(s, rows_of(fa, rows + t), floor)
        if shares is not None:
            shares.append(float(hit.mean()))
        q = rc.iterate(c, x, x if first is None or t else x + first, K, reduced)
        out.append(q)
        s, p = rc.carry(q, p, acc)
    return out


def measure_amp(c, mode, K, T, sel=START_FRAMES, acc=None, fa=None, floor=None, reduced=None, seed=0):
    """``rollout_cases.measure_amp`` with the table and the floor in the loop: the same sizes, draws and seed."""
    frames, sel = c["frames"], list(sel)
    prev = [max(f - 1, 0) for f in sel]
    x, xp = frames[sel], frames[prev]
    a = 0.0 if acc is None else np.asarray(acc)[None, None, :]
    make = lambda x, xp: ((x if mode == "zero" else 2.0 * x - xp) + a, x)
    run = lambda s, p, first=None: rollout(c, K, T, s, p, sel, acc, fa, floor, reduced, first)
    base = run(*make(x, xp))
    rng = np.random.default_rng(seed)
    amp = np.zeros(T)
    for size in (1e-9, 1e-12):
        for _ in range(3):
            runs = [run(*make(x + size * rng.standard_normal(x.shape), xp + size * rng.standard_normal(x.shape)))]
            runs.append(run(*make(x, xp), first=size * rng.standard_normal(x.shape)))
            for got in runs:
                for t in range(T):
                    amp[t] = max(amp[t], float(np.abs(got[t] - base[t]).max() / size))
    return np.maximum.accumulate(amp)


def ext_bound(x, fa):
    """eps (|x| + |fa|): the one rounding of x = fl(s + fa), as one number over the tensors."""
    return EPS * (float(np.abs(x).max()) + (0.0 if fa is None else float(np.abs(fa).max())))


def bound_T(one, K, T, amp, ref, acc, fa):
    """B of the module docstring for a result ``ref`` (its size stands for |q|, |p| and |x|)."""
    return rc.bound_T(one, K, T, amp, rc.adv_bound(ref, ref, acc) + ext_bound(ref, fa))


def check_shares(shares):
    """The condition of the module docstring on the stored shares of one floor case, (steps,)."""
    shares = np.asarray(shares, dtype=np.float64)
    assert shares.size and (shares >= SHARE[0]).all() and (shares <= SHARE[1]).all(), shares


# ------------------------------------------------------------------ the roll-out whose state lives in z
def z_model(s, ops, acc, fa):
    """``zroll_model.ZModel`` with a force table: per coordinate Phi_d = W_d (D fa_d) (r x rows) joins c_z, and the first iterate of a
    step is q^0 = o + a + U y + fa[row] (the engine forms it on the touched rows only).  ``fa`` (N, 3) or (T_s, N, 3), float64;
    ``rollout(z0, zm1, K, T, rows, frows)``: ``frows`` the table rows of step 1, one per frame (ignored for a constant table)."""
    from gsub_model import LD
    from zroll_model import ZModel

    class ZForces(ZModel):
        def __init__(self):
            ZModel.__init__(self, s, ops, acc)
            self.fa = np.asarray(fa, dtype=np.float64)

        def _fa(self, frows):
            return np.broadcast_to(self.fa[None], (len(frows),) + self.fa.shape) if self.fa.ndim == 2 else self.fa[np.asarray(frows, dtype=np.int64)]

        def step(self, z, zp, K, rows=None, frows=None):
            from pins_cases import targets
            f = self._fa(frows).astype(LD)                          # (F, N, 3)
            y = 2 * z - zp
            tgt = None if self.pins is None else np.asarray(targets(self.s, rows), dtype=np.float64)
            cz = []
            for d in range(3):
                c = self.kappa[d][None, :] + y[:, :, d] @ self.T[d].T
                if tgt is not None:
                    c = c + tgt[:, :, d].astype(LD) @ self.E[d].T
                cz.append(c + (self.D[None, :] * f[:, :, d]) @ self.g.W[d].T)
            q = self.expand(y, self.a) + f
            zi, its = y, []
            for _ in range(K):
                co = self.coefficients(q.astype(np.float64))
                zi = np.stack([cz[d] + sum(co[i][0][d].T.astype(LD) @ self.G[i][d].T for i in sorted(self.ops)) for d in range(3)], axis=2)
                q = self.expand(zi)
                its.append(dict(coef={i: co[i][0] for i in co}, P={i: co[i][1] for i in co}, z=zi.astype(np.float64)))
            return zi, dict(y=y.astype(np.float64), zp=zp.astype(np.float64), z_in=z.astype(np.float64), tgt=tgt, its=its,
                            f=np.asarray(f, dtype=np.float64))

        def rollout(self, z0, zm1, K, T, rows=None, frows=None):
            z, zp, out, recs = np.asarray(z0, dtype=LD), np.asarray(zm1, dtype=LD), [], []
            for t in range(T):
                zn, rec = self.step(z, zp, K, None if rows is None else np.asarray(rows, dtype=np.int64) + t,
                                    np.asarray(frows, dtype=np.int64) + t)
                out.append(zn)
                recs.append(rec)
                z, zp = zn, z
            return out, recs

    return ZForces()


def z_force_bound(zm, rec):
    """What the force adds to one step of the roll-out in z, as an error in q, beside ``zroll_cases.one_bound`` (whose terms it does
    not touch): Phi[:, row] is one more term of c_z -- its reduce is a chain of length N per entry with W = fl(U At^-1)^T, the form of
    ``zroll_cases``' once-per-call terms, (N + 2 r + 16) eps |U| |At^-1| |U^T| (D |fa|) and 64 eps kappa(At_d) |U| |W D fa|, and it joins
    kappa with one rounding, eps |U| (|kappa| + |Phi|) -- and the add on the touched rows rounds once, eps (|q^0| + |fa|)."""
    from gsub_model import EPS as E, LD
    g = zm.g
    f = rec["f"]
    D = zm.D.astype(np.float64)
    worst = 0.0
    for d in range(3):
        aU = np.abs(g.U[d]).astype(np.float64)
        R = (D[None, :] * f[:, :, d]).T                             # (N, F)
        phi = np.asarray(g.W[d] @ R.astype(LD))
        chain = (g.N + 2 * g.r + 16) * E * float((aU @ (np.abs(g.Ai[d]).astype(np.float64) @ (aU.T @ np.abs(R)))).max())
        inv = 64 * E * g.kappa[d] * float((aU @ np.abs(phi).astype(np.float64)).max())
        join = E * float((aU @ (np.abs(zm.kappa[d]).astype(np.float64)[:, None] + np.abs(phi).astype(np.float64))).max())
        q0 = float((np.abs(g.o[:, d]).astype(np.float64)[None, :] + abs(float(zm.a[d])) + np.abs(rec["y"][:, :, d]) @ aU.T).max())
        worst = max(worst, chain + inv + join + E * (q0 + float(np.abs(f[:, :, d]).max())))
    return worst
