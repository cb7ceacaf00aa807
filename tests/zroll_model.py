"""Shared by tests/test_zroll_cpu.py and tests/test_gpu_zroll.py: the host model of a roll-out whose state lives in the coordinates
z of a position subspace q = o + U z (csrc/asb_zroll.hip), in numpy.longdouble, built on ``gsub_model.Galerkin``
(U, At = U^T A U, W = At^-1 U^T, A o), ``projections.project_host`` (the projections, in float64 at the float64 iterate, as
``pdsolve_cases.reduced_term`` takes them) and ``pins_cases.targets``.

Per coordinate d, with D = diag(masses / dt^2) and a = dt^2 g:

    T = W D U (r x r)      kappa = W (D (o + a 1) - A o) (r)      E[:, i] = w_i W[:, v_i] (r x P)      G_k = W S_k^T V_k (r x m_k)

    start    z_0 = U^T (x_f - o),  z_-1 = U^T (x_{f-1} - o)  (or z_0)
    step     y = 2 z_t - z_{t-1};  c_z = kappa + T y + E target(row);  q^0 = o + a + U y;
             K times: coef_k = H_k p_k(q)[Pt_k] for every kind from the OLD q, z = c_z + sum_k G_k coef_k, q = o + U z;  z_{t+1} = z

``ZModel.rollout`` returns every z_t and, per step, what the bounds of tests/zroll_cases.py are sized by (``records``)."""
import numpy as np

from gsub_model import LD


class ZModel(object):
    def __init__(self, s, ops, acc=None):
        """``s``: a case of ``gsub_cases.sub_case`` (``galerkin``, ``kinds``, ``masses``, ``dt``; with ``pins`` of
        ``pins_cases.with_pins`` its matrix holds their weights); ``ops``: {index of a kind: its ``ReducedOperator``}, EVERY
        kind of the case; ``acc`` = dt^2 g."""
        assert sorted(ops) == list(range(len(s["kinds"]))), "every kind is reduced"
        self.s, self.g, self.ops = s, s["galerkin"], dict(ops)
        g = self.g
        self.a = np.zeros(3, dtype=LD) if acc is None else np.asarray(acc, dtype=np.float64).astype(LD)
        self.D = (np.asarray(s["masses"], dtype=np.float64) / s["dt"] ** 2).astype(LD)
        self.T = [g.W[d] @ (self.D[:, None] * g.U[d]) for d in range(3)]
        self.const = [self.D * (g.o[:, d] + self.a[d]) - g.Ao[:, d] for d in range(3)]      # (N): D (o + a) - A o
        self.kappa = [g.W[d] @ self.const[d] for d in range(3)]
        self.M = {i: [np.asarray(s["kinds"][i][1] @ op.V[:, :, d], dtype=np.float64).astype(LD) for d in range(3)] for i, op in self.ops.items()}
        self.G = {i: [g.W[d] @ self.M[i][d] for d in range(3)] for i in self.ops}
        self.pins = s.get("pins")
        self.E = None
        if self.pins is not None:
            v, w = self.pins[0], self.pins[1].astype(LD)
            self.E = [g.W[d][:, v] * w[None, :] for d in range(3)]

    # ---- coordinates and expansion
    def coordinates(self, x):
        """(F, N, 3) -> z (F, r, 3) = U^T (x - o), longdouble."""
        x = np.asarray(x, dtype=np.float64).astype(LD)
        return np.stack([(x[:, :, d] - self.g.o[None, :, d]) @ self.g.U[d] for d in range(3)], axis=2)

    def expand(self, z, a=None):
        """z (F, r, 3) -> o (+ a) + U z, (F, N, 3) longdouble."""
        q = np.stack([self.g.o[None, :, d] + z[:, :, d] @ self.g.U[d].T for d in range(3)], axis=2)
        return q if a is None else q + a[None, None, :]

    def project(self, x):
        """x projected into o + span(U), rounded to float64."""
        return self.expand(self.coordinates(x)).astype(np.float64)

    def start(self, frames, sel, mode):
        """(z_0, z_-1) of the selected frames (frame 0 takes x_0 as its previous frame)."""
        sel = list(sel)
        z0 = self.coordinates(frames[sel])
        return z0, (z0.copy() if mode == "zero" else self.coordinates(frames[[max(f - 1, 0) for f in sel]]))

    # ---- a step
    def coefficients(self, q64):
        """{index: (coef (3, m, F) float64, P (F, |Pt|, 3))} at the float64 iterate."""
        from animsnapbases_amd import projections as proj
        out = {}
        for i, op in self.ops.items():
            setup, _, smin, smax = self.s["kinds"][i]
            P = proj.project_host(setup, q64, smin, smax)[:, op.Pt]
            out[i] = (np.stack([op.H[d] @ P[:, :, d].T for d in range(3)]), P)
        return out

    def step(self, z, zp, K, rows=None):
        """One time step: (z_{t+1}, record); ``rows``: the rows of the pins' shift, one per frame."""
        from pins_cases import targets
        y = 2 * z - zp
        tgt = None if self.pins is None else np.asarray(targets(self.s, rows), dtype=np.float64)
        cz = []
        for d in range(3):
            c = self.kappa[d][None, :] + y[:, :, d] @ self.T[d].T
            if tgt is not None:
                c = c + tgt[:, :, d].astype(LD) @ self.E[d].T
            cz.append(c)
        q = self.expand(y, self.a)
        zi, its = y, []
        for _ in range(K):
            co = self.coefficients(q.astype(np.float64))
            zi = np.stack([cz[d] + sum(co[i][0][d].T.astype(LD) @ self.G[i][d].T for i in sorted(self.ops)) for d in range(3)], axis=2)
            q = self.expand(zi)
            its.append(dict(coef={i: co[i][0] for i in co}, P={i: co[i][1] for i in co}, z=zi.astype(np.float64)))
        return zi, dict(y=y.astype(np.float64), zp=zp.astype(np.float64), z_in=z.astype(np.float64), tgt=tgt, its=its)

    def rollout(self, z0, zm1, K, T, rows=None):
        """([z_1, .., z_T] longdouble, [record of step t]); ``rows``: the rows of step 1, step t reads rows + t - 1."""
        z, zp, out, recs = np.asarray(z0, dtype=LD), np.asarray(zm1, dtype=LD), [], []
        for t in range(T):
            zn, rec = self.step(z, zp, K, None if rows is None else np.asarray(rows, dtype=np.int64) + t)
            out.append(zn)
            recs.append(rec)
            z, zp = zn, z
        return out, recs
