"""Shared by tests/test_gsub_cpu.py and tests/test_gpu_gsub.py: the host model of the global step in a position subspace
q = o + U z (csrc/asb_gsub.hip), in numpy.longdouble (the x87 format here: 64-bit mantissa).

Per coordinate d, for a basis U_d (N x r) of full column rank and an origin o, the Galerkin step is

    q_d = o_d + U_d (U_d^T A U_d)^-1 U_d^T (rhs_d - A o_d)  =  o'_d + P_d rhs_d.

``Galerkin`` holds U, At = U^T A U and its inverse in longdouble (a float64 inverse refined by three Newton steps
X <- X (2 I - At X) in longdouble: what remains is eps_ld kappa(At), 2^-11 of what a float64 inverse can reach) and offers

    solve(b)            b (N, 3) -> q (N, 3) float64: the object ``pdsolve_cases.model`` takes in place of its ``lu``
    apply(R, affine)    R (3 N, w) vertex-major (row 3 v + d) -> the same layout, longdouble: what asb_test_gsub_apply computes
    magnitude(R)        |U| (|At^-1| (|U^T| |R|)) entry by entry: the size of the terms the two dot-product chains add up
    coefficients(R)     |U| |z|, z = At^-1 U^T R: the size of what the r x r inverse's error is multiplied with

The device orthonormalises U per coordinate first (``projections.subspace_basis``); the projection depends on the span alone, so
the model may hold either."""
import numpy as np

LD = np.longdouble
EPS = np.finfo(np.float64).eps


def _inverse_ld(M):
    """M^-1 in longdouble for a small symmetric positive definite M (longdouble)."""
    X = np.linalg.inv(M.astype(np.float64)).astype(LD)
    eye2 = 2 * np.eye(M.shape[0], dtype=LD)
    for _ in range(3):
        X = X @ (eye2 - M @ X)
    return 0.5 * (X + X.T)


class Galerkin(object):
    def __init__(self, A, Qt, origin):
        """``A``: scipy sparse or dense (N, N); ``Qt`` (3, r, N): U_d^T per coordinate; ``origin`` (N, 3)."""
        self.A = (A.toarray() if hasattr(A, "toarray") else np.asarray(A)).astype(LD)
        self.U = [np.asarray(Qt[d], dtype=np.float64).T.astype(LD) for d in range(3)]
        self.o = np.asarray(origin, dtype=np.float64).astype(LD)
        self.N, self.r = self.U[0].shape
        self.At = [U.T @ self.A @ U for U in self.U]
        self.Ai = [_inverse_ld(At) for At in self.At]
        self.W = [Ai @ U.T for Ai, U in zip(self.Ai, self.U)]                      # (r, N)
        self.Ao = self.A @ self.o
        self.op = np.stack([self.o[:, d] - self.U[d] @ (self.W[d] @ self.Ao[:, d]) for d in range(3)], axis=1)
        self.kappa = [float(np.linalg.cond(At.astype(np.float64))) for At in self.At]

    def P(self, d):
        return self.U[d] @ self.W[d]

    def solve(self, b):
        b = np.asarray(b, dtype=np.float64).astype(LD)
        return np.stack([self.op[:, d] + self.U[d] @ (self.W[d] @ b[:, d]) for d in range(3)], axis=1).astype(np.float64)

    def apply(self, R, affine=True):
        R = np.asarray(R, dtype=np.float64).astype(LD)
        out = np.empty(R.shape, dtype=LD)
        for d in range(3):
            out[d::3] = self.U[d] @ (self.W[d] @ R[d::3]) + (self.op[:, d][:, None] if affine else 0)
        return out

    def magnitude(self, R):
        R = np.abs(np.asarray(R, dtype=np.float64))
        out = np.empty(R.shape)
        for d in range(3):
            U = np.abs(self.U[d]).astype(np.float64)
            out[d::3] = U @ (np.abs(self.Ai[d]).astype(np.float64) @ (U.T @ R[d::3]))
        return out

    def coefficients(self, R):
        R = np.asarray(R, dtype=np.float64).astype(LD)
        out = np.empty(R.shape)
        for d in range(3):
            out[d::3] = (np.abs(self.U[d]) @ np.abs(self.W[d] @ R[d::3])).astype(np.float64)
        return out

    def residual(self, Q, R):
        """max_d max |U_d^T (A q_d - rhs_d)| of a result ``Q`` for the right-hand side ``R`` (both (3 N, w)), in longdouble."""
        Q, R = np.asarray(Q).astype(LD), np.asarray(R, dtype=np.float64).astype(LD)
        return max(float(np.abs(self.U[d].T @ (self.A @ Q[d::3] - R[d::3])).max()) for d in range(3))


def vertex_major(X):
    """(F, N, 3) frame-major -> (3 N, F), row 3 v + d."""
    X = np.asarray(X)
    return np.ascontiguousarray(X.transpose(1, 2, 0).reshape(3 * X.shape[1], X.shape[0]))


def svd_basis(frames, r=None):
    """The fixtures' basis: origin = frame 0 and, per coordinate, the leading right singular vectors of frames - frame 0, as a
    world-space (K, N, 3) array (K = r, or all min(F, N) of them)."""
    frames = np.asarray(frames, dtype=np.float64)
    N = frames.shape[1]
    K = min(N, frames.shape[0]) if r is None else r
    comps = np.empty((K, N, 3))
    for d in range(3):
        comps[:, :, d] = np.linalg.svd(frames[:, :, d] - frames[0, :, d][None], full_matrices=False)[2][:K]
    return comps
