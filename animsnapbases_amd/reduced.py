"""The reduced constraint operator of the reference's projective-dynamics simulator, restated on the host (NumPy / SciPy, no
engine): what ``prepare_reduced_group`` (projective_dynamics/Simulators.py:157-220) and ``prepare_reduced_verts_bending``
(:222-255) build from the ``.npz`` of ``store_components_n_interpol_points`` -- without the dense ``assembly_ST.toarray()``:
the product S^T V is left to the caller (``St @ V_d`` sparse on the host, ``asb_rforce_operator`` on the device).

Per coordinate d the reduced term of one frame is ``(S^T V_d) H_d p_d[sampled rows]`` (``get_group_reduced_term``, :366-399)
with ``H_d = (A^T A + la_d I)^-1 A^T``, ``A = V_d[Pt]`` -- the explicit form of the reference's
``lu_solve(lu_factor(AtA + la I), PtV^T @ p)``, as ``constraintsComponents.interpolation_errors`` already forms it.
"""
import numpy as np

# constraint_projection_reduction_type -> rows of a sampled element that are kept: one ("row") or all p ("block")
REDUCTIONS = {"deim_pod": "row", "deim_pod_vectorized": "row", "deim_pca_blocks": "block", "geom_pca_blocks_withSt": "block"}
BASIS_KEYS = ("components", "interpol_alphas", "Pt", "interpol_alpha_ranges")


class ReducedOperator(object):
    """``elements`` (n,): the sampled elements, in the order their projections are stacked (an element sampled twice is
    listed twice); ``Pt`` (|Pt|,): the sampled rows of the full stack (rows of V); ``local_rows`` (|Pt|,): the same rows in
    the stack of the sampled elements alone (row i p + l of the i-th entry of ``elements``); ``V`` (rows, mp, 3);
    ``H`` (3, mp, |Pt|); ``la`` (3,) the Tikhonov terms; ``cond`` (3,) the condition numbers of A^T A + la I."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def reduced_operator(components, interpol_alphas, Pt, interpol_alpha_ranges, num_components, p, reduction="deim_pod",
                     n_elements=None, verts_bending=False):
    """``components`` (K, rows, 3), ``interpol_alphas``, ``Pt``, ``interpol_alpha_ranges``: the four keys the simulator loads
    (:179-188); ``num_components`` = m; ``p``: rows per element of the kind; ``reduction``: one of ``REDUCTIONS``;
    ``n_elements``: the elements of the kind (default rows // p).  ``verts_bending``: the path of :222-255 -- ``Pt`` serves as
    both the elements (positions in the list of constrained vertices) and the rows, one row each, no Tikhonov term.

    Raises ValueError for an unknown reduction, m outside 1..K or beyond the ranges, fewer sampled rows than basis vectors, a
    point outside the rows or elements, and a basis whose rows are not elements x p."""
    from scipy.linalg import lu_factor, lu_solve
    if reduction not in REDUCTIONS:
        raise ValueError("unknown reduction %r: one of %s" % (reduction, ", ".join(sorted(REDUCTIONS))))
    comps = np.asarray(components, dtype=np.float64)
    if comps.ndim != 3 or comps.shape[2] != 3:
        raise ValueError("components of shape %s: (K, rows, 3) expected" % (comps.shape,))
    K, rows = int(comps.shape[0]), int(comps.shape[1])
    p = int(p)
    if verts_bending and p != 1:
        raise ValueError("verts_bending has p = 1, not %d" % p)
    n_elements = rows // p if n_elements is None else int(n_elements)
    if rows != n_elements * p:
        raise ValueError("the basis has %d rows, %d elements x %d expected" % (rows, n_elements, p))
    row_dim = 1 if (verts_bending or REDUCTIONS[reduction] == "row") else p
    m = int(num_components)
    if m < 1 or m * row_dim > K:
        raise ValueError("r = %d is outside 1..%d" % (m, K // row_dim))
    ranges = None if interpol_alpha_ranges is None else np.asarray(interpol_alpha_ranges, dtype=np.int64).reshape(-1)
    if ranges is None or ranges.shape[0] == 0:
        raise ValueError("no interpolation points: run deim() or a block interpolation first")
    if m > ranges.shape[0]:
        raise ValueError("r = %d: interpolation points exist for r <= %d only" % (m, ranges.shape[0]))
    n_alpha = int(ranges[m - 1])
    mp = m * row_dim
    if row_dim == 1:                                    # (:187-188, :236) the stored rows; (:384-386) row Pt % p of the element
        rows_pt = np.asarray(Pt, dtype=np.int64).reshape(-1)[:n_alpha]
        alphas = rows_pt if verts_bending else np.asarray(interpol_alphas, dtype=np.int64).reshape(-1)[:n_alpha]
        if alphas.shape[0] != rows_pt.shape[0]:
            raise ValueError("r = %d: %d interpolation elements for %d interpolation rows" % (m, alphas.shape[0], rows_pt.shape[0]))
        local = np.arange(rows_pt.shape[0], dtype=np.int64) * p + rows_pt % p
    else:                                               # (:190-193) every row of the sampled blocks
        alphas = np.asarray(interpol_alphas, dtype=np.int64).reshape(-1)[:n_alpha]
        rows_pt = (alphas[:, None] * p + np.arange(p, dtype=np.int64)[None, :]).reshape(-1)
        local = np.arange(rows_pt.shape[0], dtype=np.int64)
    if rows_pt.shape[0] < mp:
        raise ValueError("r = %d: %d interpolation rows for %d basis vectors: the normal matrix is singular" % (m, rows_pt.shape[0], mp))
    if alphas.size and (alphas.min() < 0 or alphas.max() >= n_elements):
        bad = int(alphas.max()) if alphas.max() >= n_elements else int(alphas.min())
        raise ValueError("an interpolation point names element %d, the kind has elements 0..%d" % (bad, n_elements - 1))
    if rows_pt.min() < 0 or rows_pt.max() >= rows:
        bad = int(rows_pt.max()) if rows_pt.max() >= rows else int(rows_pt.min())
        raise ValueError("an interpolation point names row %d, the basis has rows 0..%d" % (bad, rows - 1))
    V = np.ascontiguousarray(comps.swapaxes(0, 1)[:, :mp, :])           # (:180-181) (rows, mp, 3)
    PtV = V[rows_pt]                                                    # (|Pt|, mp, 3)
    AtA = np.einsum('nai,ami->nmi', PtV.swapaxes(0, 1), PtV)            # (:207)
    la = np.zeros(3) if verts_bending else 1e-8 * np.trace(AtA) / AtA.shape[0]      # (:209; none at :253-255)
    H, cond = np.empty((3, mp, rows_pt.shape[0])), np.empty(3)
    for d in range(3):                                                  # (:211-214)
        G = AtA[:, :, d] + la[d] * np.eye(mp)
        H[d] = lu_solve(lu_factor(G), PtV[:, :, d].T)
        cond[d] = np.linalg.cond(G)
    return ReducedOperator(reduction=reduction, num_components=m, p=p, row_dim=row_dim, elements=alphas.copy(), Pt=rows_pt,
                           local_rows=local, V=V, H=H, la=np.asarray(la, dtype=np.float64), cond=cond)


def load_basis(basis):
    """The four keys of ``BASIS_KEYS`` from a ``constraintsComponents`` with components and interpolation points, the path
    of its stored ``.npz`` or a dict."""
    if isinstance(basis, (str, bytes)) or hasattr(basis, "__fspath__"):
        with np.load(basis, allow_pickle=False) as z:
            missing = [k for k in BASIS_KEYS if k not in z.files]
            if missing:
                raise ValueError("%s has no %r (the keys of store_components_n_interpol_points)" % (basis, missing[0]))
            return {k: z[k] for k in BASIS_KEYS}
    if isinstance(basis, dict):
        missing = [k for k in BASIS_KEYS if k not in basis]
        if missing:
            raise ValueError("the basis dict has no %r (the keys of store_components_n_interpol_points)" % (missing[0],))
        return {k: basis[k] for k in BASIS_KEYS}
    if getattr(basis, "geom_alpha_ranges", None) is None or len(basis.geom_alpha_ranges) == 0:
        raise ValueError("no interpolation points: run deim() or a block interpolation first")
    return {"components": basis.comps, "interpol_alphas": basis.geom_alpha, "Pt": basis.geom_Pt,
            "interpol_alpha_ranges": basis.geom_alpha_ranges}
