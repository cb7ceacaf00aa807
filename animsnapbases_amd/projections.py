"""Rest-pose set-up of the reference's five element projections (projective_dynamics/Constraint_projections.py), restated
from their definitions for the device kernel of csrc/asb_cproj.hip, plus a NumPy restatement of the per-frame projection
(``project_host``) that the timing tool uses for scale.

Per element kind: p rows per element, the index width and the per-element table the kernel reads.

  kind                        p  indices  table (doubles per element)
  edge_spring                 1  (E, 2)   1: rest length d (:280)
  tris_strain                 2  (T, 3)   10: the 3 x 2 frame P (:368-376) row-major, then the 2 x 2 DmInv (:379-381)
  tets_strain                 3  (T, 4)   9: DmInv of Dm = [p1 - p4, p2 - p4, p3 - p4] (:496-505)
  tets_deformation_gradient   3  (T, 4)   9: the same DmInv (:635-639)
  verts_bending               1  (n, 1)   5: rest mean-curvature norm, averaged triangle normal, dot_with_normal (:178-186);
                                          behind the n x 5 block the cotangent weights / Voronoi-area third of every star
                                          edge (:156-169), in the order of the star CSR

The star CSR of ``verts_bending`` lists, per constrained vertex, the neighbour ``v2`` of every star edge in the order
``DeformableMesh.vertex_star`` finds them (:1129-1162): the per-frame sum (:201-202) runs in that order.

Every projection is a function of the deformation gradient itself: no singular vector is returned, so the sign and ordering
choices of an SVD routine never show.
"""
import collections

import numpy as np

# kind -> (p, vertices per element, table doubles per element, code of the C ABI)
KINDS = {
    "edge_spring": (1, 2, 1, 0),
    "tris_strain": (2, 3, 10, 1),
    "tets_strain": (3, 4, 9, 2),
    "tets_deformation_gradient": (3, 4, 9, 3),
    "verts_bending": (1, 1, 5, 4),
}


class ProjectionSetup(object):
    """What ``asb_cproj_setup`` uploads: ``idx`` (n, width) int64, ``table`` (flat float64), for ``verts_bending`` the star
    CSR ``star_ptr`` (n + 1) / ``star_idx`` (nnz) and ``bending_indices`` (the constrained vertices, Simulators.py:312)."""

    def __init__(self, kind, idx, table, star_ptr=None, star_idx=None, bending_indices=None, parts=None):
        self.kind = kind
        self.p, self.width, self.table_width, self.code = KINDS[kind]
        self.idx = np.ascontiguousarray(idx, dtype=np.int64)
        self.table = np.ascontiguousarray(table, dtype=np.float64).reshape(-1)
        self.star_ptr = None if star_ptr is None else np.ascontiguousarray(star_ptr, dtype=np.int64)
        self.star_idx = None if star_idx is None else np.ascontiguousarray(star_idx, dtype=np.int64)
        self.bending_indices = bending_indices
        self.parts = parts or {}            # the named rest tables (tests, project_host)
        self.n_elem = int(self.idx.shape[0])
        self.rows = self.n_elem * self.p


def _check_elements(kind, elements, n_verts):
    width = 3 if kind == "verts_bending" else KINDS[kind][1]
    el = np.asarray(elements)
    if el.ndim != 2 or el.shape[1] != width:
        raise ValueError("%s: elements of shape %s, (n, %d) expected" % (kind, el.shape, width))
    if el.shape[0] < 1:
        raise ValueError("%s: no elements" % kind)
    if not np.issubdtype(el.dtype, np.integer):
        raise ValueError("%s: elements must be integers, not %s" % (kind, el.dtype))
    el = el.astype(np.int64)
    if el.min() < 0 or el.max() >= n_verts:
        bad = int(el.max()) if el.max() >= n_verts else int(el.min())
        raise ValueError("%s: an element names vertex %d, the animation has vertices 0..%d" % (kind, bad, n_verts - 1))
    return el


def edge_spring_tables(rest, edges):
    """Rest length d = |x_v0 - x_v1| (:279-280)."""
    d = np.linalg.norm(rest[edges[:, 0]] - rest[edges[:, 1]], axis=1)
    if (d == 0).any():
        raise ValueError("edge_spring: degenerate rest element %d: rest edge length is 0" % int(np.flatnonzero(d == 0)[0]))
    return d


def tris_strain_tables(rest, tris):
    """The tangent frame P (3 x 2: the normalised first edge, the second edge orthogonalised against it, :368-376) and the
    inverse of the rest edges in that frame (:379-381)."""
    p1, p2, p3 = rest[tris[:, 0]], rest[tris[:, 1]], rest[tris[:, 2]]
    e1, e2 = p2 - p1, p3 - p1
    n1 = np.linalg.norm(e1, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        c0 = e1 / n1[:, None]
        c1 = e2 - np.einsum("ij,ij->i", e2, c0)[:, None] * c0
        n2 = np.linalg.norm(c1, axis=1)
        c1 = c1 / n2[:, None]
    P = np.stack([c0, c1], axis=2)                                  # (T, 3, 2)
    Dm = np.einsum("tij,tik->tjk", P, np.stack([e1, e2], axis=2))   # P^T [e1 e2]  (T, 2, 2)
    det = Dm[:, 0, 0] * Dm[:, 1, 1] - Dm[:, 0, 1] * Dm[:, 1, 0]
    bad = ~(np.isfinite(det) & (det != 0))
    if bad.any():
        raise ValueError("tris_strain: degenerate rest element %d: |det Dm| is 0" % int(np.flatnonzero(bad)[0]))
    return P, np.linalg.inv(Dm)


def tets_tables(rest, tets, kind="tets_strain"):
    """DmInv of Dm = [p1 - p4, p2 - p4, p3 - p4] as columns (:502-504, :638-639)."""
    p4 = rest[tets[:, 3]]
    Dm = np.stack([rest[tets[:, 0]] - p4, rest[tets[:, 1]] - p4, rest[tets[:, 2]] - p4], axis=2)
    det = np.linalg.det(Dm)
    if (det == 0).any():
        raise ValueError("%s: degenerate rest element %d: |det Dm| is 0" % (kind, int(np.flatnonzero(det == 0)[0])))
    return np.linalg.inv(Dm)


def tris_rest_area(rest, tris, P):
    """A0 = det(P^T [p2 - p1, p3 - p1]) / 2, the signed rest area in the tangent frame (:383)."""
    e = np.stack([rest[tris[:, 1]] - rest[tris[:, 0]], rest[tris[:, 2]] - rest[tris[:, 0]]], axis=2)
    return 0.5 * np.linalg.det(np.einsum("tij,tik->tjk", P, e))


def tets_rest_volume(rest, tets):
    """V0 = det(Dm) / 6, the signed rest volume (:506, :640)."""
    p4 = rest[tets[:, 3]]
    return np.linalg.det(np.stack([rest[tets[:, 0]] - p4, rest[tets[:, 1]] - p4, rest[tets[:, 2]] - p4], axis=2)) / 6.0


def vertex_stars(tris, n_verts):
    """Per vertex the star edges [v2, vOtherT1, t1, vOtherT2, t2] in the order ``DeformableMesh.vertex_star`` appends them
    (:1129-1162): triangles in order, their corners in order, the two other corners in order; a second triangle on a known
    neighbour fills (t2, vOtherT2), a later one overwrites them."""
    stars = [[] for _ in range(n_verts)]
    where = [dict() for _ in range(n_verts)]
    for t, tri in enumerate(np.asarray(tris, dtype=np.int64)):
        for v in range(3):
            vi = int(tri[v])
            for ov in range(3):
                if ov == v:
                    continue
                nb, third = int(tri[ov]), int(tri[3 - (v + ov)])
                k = where[vi].get(nb)
                if k is None:
                    where[vi][nb] = len(stars[vi])
                    stars[vi].append([nb, third, t, -1, -1])
                else:
                    stars[vi][k][3], stars[vi][k][4] = third, t
    return stars


def _angle_at(a, b, c):
    """Angle at b between (a - b) and (c - b) (:138-143)."""
    u, v = a - b, c - b
    return np.arccos(np.clip(np.dot(u, v) / (np.linalg.norm(u) * np.linalg.norm(v)), -1, 1))


def bending_tables(rest, tris):
    """``add_vertex_bending_constraint`` (:1196-1223): the vertices whose star edges all have two triangles, and per such
    vertex the cotangent weights over a third of the incident triangle area (:156-169, :1086-1104), the norm of the rest
    mean-curvature vector, the average of the star triangles' unit normals and its product with that vector (:178-186)."""
    rest = np.asarray(rest, dtype=np.float64)
    tris = np.asarray(tris, dtype=np.int64)
    n = rest.shape[0]
    area = np.zeros(n)
    for tri in tris:                                                # (:1095-1104)
        a = 0.5 * np.linalg.norm(np.cross(rest[tri[1]] - rest[tri[0]], rest[tri[2]] - rest[tri[0]])) / 3.0
        for vi in tri:
            area[vi] += a
    area[area < 1e-7] = 1e-7
    stars = vertex_stars(tris, n)
    ids, ptr, v2s, wts, rmc, nrm, dwn, vor = [], [0], [], [], [], [], [], []
    for v in range(n):
        star = stars[v]
        if not star or any(e[4] < 0 for e in star):
            continue
        w, seen, tl = [], set(), []
        for nb, o1, t1, o2, t2 in star:
            cot = 0.5 / np.tan(_angle_at(rest[v], rest[o1], rest[nb])) + 0.5 / np.tan(_angle_at(rest[v], rest[o2], rest[nb]))
            w.append(cot / area[v])
            for t in (t1, t2):
                if t not in seen:
                    seen.add(t)
                    tl.append(t)
        mc = np.zeros(3)
        for (nb, _o1, _t1, _o2, _t2), wi in zip(star, w):
            mc += (rest[v] - rest[nb]) * wi
        normals = []
        for t in tl:                                                # (:145-154)
            a, b, c = rest[tris[t]]
            nn = np.cross(b - a, c - a)
            ln = np.linalg.norm(nn)
            if ln > 1e-10:
                normals.append(nn / ln)
        tn = np.mean(normals, axis=0) if normals else np.array([0.0, 0.0, 1.0])
        ids.append(v)
        v2s += [e[0] for e in star]
        wts += w
        ptr.append(len(v2s))
        rmc.append(np.linalg.norm(mc))
        nrm.append(tn)
        dwn.append(tn @ mc)
        vor.append(area[v])
    return dict(indices=np.array(ids, dtype=np.int64), star_ptr=np.array(ptr, dtype=np.int64),
                star_idx=np.array(v2s, dtype=np.int64), weights=np.array(wts, dtype=np.float64),
                rest_curvature=np.array(rmc, dtype=np.float64), normal=np.array(nrm, dtype=np.float64).reshape(-1, 3),
                dot_with_normal=np.array(dwn, dtype=np.float64), voronoi_area=np.array(vor, dtype=np.float64))


def build_setup(kind, elements, rest_positions):
    """The upload of one element kind for rest positions (N, 3).  ``elements``: the index array of the table above; for
    ``verts_bending`` the (M, 3) triangles of the mesh.  Raises ValueError for an unknown kind, a wrong element width, an index
    outside the mesh or a degenerate rest element."""
    if kind not in KINDS:
        raise ValueError("unknown projection kind %r: one of %s" % (kind, ", ".join(sorted(KINDS))))
    rest = np.asarray(rest_positions, dtype=np.float64)
    if rest.ndim != 2 or rest.shape[1] != 3:
        raise ValueError("rest positions of shape %s: (N, 3) expected" % (rest.shape,))
    el = _check_elements(kind, elements, rest.shape[0])
    if kind == "edge_spring":
        d = edge_spring_tables(rest, el)
        return ProjectionSetup(kind, el, d, parts=dict(d=d))
    if kind == "tris_strain":
        P, DmInv = tris_strain_tables(rest, el)
        table = np.concatenate([P.reshape(-1, 6), DmInv.reshape(-1, 4)], axis=1)
        return ProjectionSetup(kind, el, table, parts=dict(P=P, DmInv=DmInv, A0=tris_rest_area(rest, el, P)))
    if kind in ("tets_strain", "tets_deformation_gradient"):
        DmInv = tets_tables(rest, el, kind)
        return ProjectionSetup(kind, el, DmInv.reshape(-1, 9), parts=dict(DmInv=DmInv, V0=tets_rest_volume(rest, el)))
    b = bending_tables(rest, el)
    if b["indices"].shape[0] == 0:
        raise ValueError("verts_bending: no vertex of the mesh has a closed star (every star edge needs two triangles)")
    head = np.concatenate([b["rest_curvature"][:, None], b["normal"], b["dot_with_normal"][:, None]], axis=1)
    return ProjectionSetup(kind, b["indices"][:, None], np.concatenate([head.reshape(-1), b["weights"]]), b["star_ptr"],
                           b["star_idx"], bending_indices=b["indices"], parts=b)


def subset_setup(setup, sel):
    """The upload of the elements ``sel`` of ``setup`` alone, in that order (an element may repeat): the rest tables are taken
    over, not rebuilt, so element ``sel[i]`` projects to the same bits as in the full set-up.  For ``verts_bending`` ``sel``
    counts the constrained vertices (positions in ``bending_indices``)."""
    sel = np.asarray(sel, dtype=np.int64).reshape(-1)
    if sel.shape[0] < 1:
        raise ValueError("%s: no elements" % setup.kind)
    if sel.min() < 0 or sel.max() >= setup.n_elem:
        bad = int(sel.max()) if sel.max() >= setup.n_elem else int(sel.min())
        raise ValueError("%s: element %d of a set-up with elements 0..%d" % (setup.kind, bad, setup.n_elem - 1))
    tw, n = setup.table_width, setup.n_elem
    head = setup.table[:n * tw].reshape(n, tw)[sel]
    q = setup.parts
    if setup.kind != "verts_bending":
        return ProjectionSetup(setup.kind, setup.idx[sel], head, parts={k: v[sel] for k, v in q.items()})
    ptr, wts = setup.star_ptr, setup.table[n * tw:]
    edges = np.concatenate([np.arange(ptr[i], ptr[i + 1]) for i in sel]) if sel.size else np.zeros(0, dtype=np.int64)
    new_ptr = np.concatenate([[0], np.cumsum(ptr[sel + 1] - ptr[sel])])
    per_edge = dict(star_ptr=new_ptr, star_idx=setup.star_idx[edges], weights=wts[edges])
    parts = {k: per_edge[k] if k in per_edge else v[sel] for k, v in q.items()}
    return ProjectionSetup(setup.kind, setup.idx[sel], np.concatenate([head.reshape(-1), wts[edges]]), new_ptr,
                           setup.star_idx[edges], bending_indices=setup.bending_indices[sel], parts=parts)


def touched_setup(setup, n_verts=None, into=None):
    """``(touched, compact)`` for the hyper-reduced iterations: ``touched`` the sorted unique vertices the elements of
    ``setup`` read (their corners; for ``verts_bending`` the constrained vertices and their star neighbours), ``compact`` the
    same set-up with every vertex index replaced by its position in ``touched`` -- so that the elements project the rows
    ``q[:, touched]`` of an iterate exactly as ``setup`` projects ``q``.  The tables are taken over, not rebuilt: the same bits.
    ``bending_indices`` keeps naming the mesh's vertices.  ``n_verts`` given: ``touched`` is ``arange(n_verts)`` and the
    renumbering is the identity (every row of the iterate is kept).  ``into`` given (not with ``n_verts``): a strictly ascending
    vertex list that holds every vertex the elements read -- the union of several kinds' touched sets, ``touched_union`` --;
    ``touched`` is that list and the set-up is numbered in it, so that several kinds share the rows ``q[:, into]``."""
    star = setup.star_idx if setup.star_idx is not None else np.zeros(0, dtype=np.int64)
    if into is not None:
        if n_verts is not None:
            raise ValueError("%s: either n_verts or into" % setup.kind)
        touched = np.asarray(into, dtype=np.int64).reshape(-1)
        own = np.unique(np.concatenate([setup.idx.reshape(-1), star]))
        if touched.size < 1 or (np.diff(touched) <= 0).any():
            raise ValueError("%s: into must be a strictly ascending vertex list" % setup.kind)
        at = np.minimum(np.searchsorted(touched, own), touched.size - 1)
        if (touched[at] != own).any():
            raise ValueError("%s: an element names vertex %d, which the given list lacks" % (setup.kind, int(own[touched[at] != own][0])))
    elif n_verts is None:
        touched = np.unique(np.concatenate([setup.idx.reshape(-1), star]))
    else:
        touched = np.arange(int(n_verts), dtype=np.int64)
        if setup.idx.max() >= n_verts or (star.size and star.max() >= n_verts):
            raise ValueError("%s: an element names vertex %d of %d" % (setup.kind, int(max(setup.idx.max(), star.max() if star.size else 0)), n_verts))
    pos = lambda a: np.searchsorted(touched, a).astype(np.int64)
    parts = dict(setup.parts)
    if setup.kind == "verts_bending":
        for k in ("indices", "star_idx"):
            if k in parts:
                parts[k] = pos(parts[k])
    compact = ProjectionSetup(setup.kind, pos(setup.idx), setup.table, setup.star_ptr,
                              None if setup.star_idx is None else pos(setup.star_idx), bending_indices=setup.bending_indices, parts=parts)
    return touched, compact


def touched_union(setups):
    """The sorted unique vertices the elements of all ``setups`` read: the one list ``touched_setup(setup, into=...)`` numbers
    every kind of a multi-kind hyper-reduced solve in."""
    return np.unique(np.concatenate([touched_setup(s)[0] for s in setups]))


def assembly_ST(setup, n_verts, wi=1.0):
    """The weighted differential operator S^T of one element kind, (n_verts, setup.rows) CSR with sorted indices: what the
    reference's ``*_assembly_ST`` hold (:1221-1284), restated from the rest tables of ``build_setup``.  Column c belongs to
    row c of the stacked projections, so ``assembly_ST @ p[f]`` is the kind's term of the global step's right-hand side
    (Simulators.py:643-724).

      edge_spring   column e: -wi at v0, +wi at v1 (:285-289)
      tris_strain   columns 2 e + j: G[j] = [DmInv^T | -rowsum(DmInv^T)][j] on (v1, v2, v3), times wi |A0| (:383-405)
      tets_*        columns 3 e + j: the same with the 3 x 3 DmInv on (v1 .. v4), times wi |V0| (:505-532, :640-667)
      verts_bending column i: wi_v sum(w) at the constrained vertex, -wi_v w_j at every star neighbour (:189-195), with the
                    constraint's own weight wi_v = wi * (a third of the incident triangle area, :119, :1216)

    Entries that are exactly zero are not stored; contributions to one (row, column) are summed."""
    from scipy import sparse
    wi = float(wi)
    if not np.isfinite(wi):
        raise ValueError("%s: the constraint weight wi must be finite, not %r" % (setup.kind, wi))
    n_verts = int(n_verts)
    if setup.idx.max() >= n_verts or (setup.star_idx is not None and setup.star_idx.size and setup.star_idx.max() >= n_verts):
        raise ValueError("%s: an element names vertex %d, S^T has %d rows" % (setup.kind, int(setup.idx.max()), n_verts))
    kind, idx, q, n = setup.kind, setup.idx, setup.parts, setup.n_elem
    if kind == "edge_spring":
        row, col = idx.reshape(-1), np.repeat(np.arange(n), 2)
        val = np.tile([-wi, wi], n)
    elif kind == "verts_bending":
        ptr, w = q["star_ptr"], q["weights"]
        deg = np.diff(ptr)
        row = np.concatenate([q["indices"], q["star_idx"]])
        col = np.concatenate([np.arange(n), np.repeat(np.arange(n), deg)])
        wv = wi * q["voronoi_area"]
        val = np.concatenate([np.array([w[ptr[i]:ptr[i + 1]].sum() for i in range(n)]) * wv, -w * np.repeat(wv, deg)])
    else:
        p, nv = setup.p, setup.width
        DmInvT = np.swapaxes(q["DmInv"], 1, 2)
        G = np.concatenate([DmInvT, -DmInvT.sum(axis=2)[:, :, None]], axis=2)          # (n, p, nv): G[e, j, corner]
        G = G * wi * np.abs(q["A0"] if kind == "tris_strain" else q["V0"])[:, None, None]
        row = np.broadcast_to(idx[:, None, :], (n, p, nv)).reshape(-1)
        col = np.broadcast_to((p * np.arange(n)[:, None] + np.arange(p)[None, :])[:, :, None], (n, p, nv)).reshape(-1)
        val = G.reshape(-1)
    St = sparse.coo_matrix((val, (row, col)), shape=(n_verts, setup.rows)).tocsr()     # (sums duplicates)
    St.eliminate_zeros()
    St.sort_indices()
    return St


def pins_ST(vertices, wi, n_verts):
    """The weighted selection operator of positional constraints, (n_verts, P) CSR with wi_i at (v_i, i): what the reference's
    ``positional_assembly_ST`` holds (``PositionalConstraint.build_SiT``, Constraint_projections.py:90-92), so that
    ``pins_ST @ targets`` is the pins' term of the global step's right-hand side (Simulators.py:401-413).  ``vertices`` (P,):
    integers of 0 .. n_verts - 1, no two equal; ``wi``: a scalar or (P,), finite and >= 0."""
    from scipy import sparse
    n_verts = int(n_verts)
    v = np.asarray(vertices, dtype=np.int64).reshape(-1)
    w = np.broadcast_to(np.asarray(wi, dtype=np.float64), v.shape)
    if v.size < 1 or v.min() < 0 or v.max() >= n_verts or np.unique(v).size != v.size:
        raise ValueError("pins: the vertices must be distinct integers of 0 .. %d" % (n_verts - 1))
    if not np.isfinite(w).all() or (w < 0.0).any():
        raise ValueError("pins: every weight wi must be finite and >= 0")
    St = sparse.coo_matrix((w, (v, np.arange(v.size))), shape=(n_verts, v.size)).tocsr()
    St.sort_indices()
    return St


def global_matrix(specs, n_verts, masses, dt, pins=None):
    """The system matrix of the global step, A_N = diag(masses) / dt^2 + sum_i w_i S_i^T S_i, (n_verts, n_verts) CSR with sorted
    indices and duplicates summed.  The reference assembles kron(A_N, I_3) from the triplets of ``get_wi_SiT_AiT_Ai_Si``
    (Simulators.py:117-145): no entry couples two coordinates and the three diagonal blocks are equal, so one N x N matrix
    serves all three.  ``specs``: a non-empty list of ``(ProjectionSetup, wi)``, one per element kind; restated per kind from
    the rest tables of ``build_setup``:

      edge_spring   wi / 2 on (v0, v0) and (v1, v1), -wi / 2 on (v0, v1) and (v1, v0) (:322-333)
      tris_strain   wi |A0| G^T G on (v1, v2, v3), G = [DmInv | -rowsum(DmInv)] (2 x 3) (:431-455)
      tets_*        wi |V0| G G^T on (v1 .. v4), G = [DmInv ; -colsum(DmInv)] (4 x 3) (:559-584, :802-827)
      verts_bending wi_v s s^T, s the constraint's selection row (sum(w) at the vertex, -w_j at every star neighbour, :189-191)
                    and wi_v = wi * (a third of the incident triangle area, :119)

    ``pins``: None or ``(vertices, wi)`` of positional constraints (checked as ``pins_ST`` checks them): wi_i is added at
    (v_i, v_i), the triplets of ``PositionalConstraint.get_wi_SiT_AiT_Ai_Si`` (:106-113); the pattern does not change.

    The reference drops triplets of |value| <= 1e-12 before summing; here nothing is dropped (the matrix stays linear in wi).
    Both triangles are averaged, so the result is symmetric to the bit.  Raises ValueError for a ``dt`` that is not finite and
    positive, ``masses`` of another shape than (n_verts,) or not finite and positive, a ``wi`` that is not finite, an empty
    list, or an element outside the matrix."""
    from scipy import sparse
    if not isinstance(specs, (list, tuple)) or len(specs) == 0:
        raise ValueError("global_matrix: specs must be a non-empty list of (setup, wi), not %r" % (specs,))
    try:
        h = float(dt)
    except (TypeError, ValueError):
        raise ValueError("global_matrix: the time step dt must be a positive number, not %r" % (dt,))
    if not np.isfinite(h) or h <= 0.0:
        raise ValueError("global_matrix: the time step dt must be finite and positive, not %r" % (dt,))
    n_verts = int(n_verts)
    m = np.asarray(masses, dtype=np.float64)
    if m.shape != (n_verts,):
        raise ValueError("global_matrix: masses of shape %s: (%d,) expected" % (m.shape, n_verts))
    if not np.isfinite(m).all() or (m <= 0.0).any():
        raise ValueError("global_matrix: every vertex mass must be finite and positive")
    diag = np.arange(n_verts, dtype=np.int64)
    rows, cols, vals = [diag], [diag], [m * (1.0 / (h * h))]
    if pins is not None:
        St = pins_ST(pins[0], pins[1], n_verts).tocoo()
        rows.append(St.row.astype(np.int64))
        cols.append(St.row.astype(np.int64))
        vals.append(St.data)
    for spec in specs:
        try:
            setup, wi = spec
            wi = float(wi)
        except (TypeError, ValueError):
            raise ValueError("global_matrix: every entry of specs is a (setup, wi) pair, not %r" % (spec,))
        if not isinstance(setup, ProjectionSetup):
            raise ValueError("global_matrix: every entry of specs is a (setup, wi) pair, not %r" % (spec,))
        if not np.isfinite(wi):
            raise ValueError("%s: the constraint weight wi must be finite, not %r" % (setup.kind, wi))
        kind, idx, q, n = setup.kind, setup.idx, setup.parts, setup.n_elem
        if idx.max() >= n_verts or (setup.star_idx is not None and setup.star_idx.size and setup.star_idx.max() >= n_verts):
            raise ValueError("%s: an element names vertex %d, the matrix has %d rows" % (kind, int(idx.max()), n_verts))
        if kind == "verts_bending":
            S = assembly_ST(setup, n_verts, 1.0)                    # column i: voronoi_area_i * s_i
            K = (S @ sparse.diags(wi / q["voronoi_area"]) @ S.T).tocoo()
            rows.append(K.row.astype(np.int64))
            cols.append(K.col.astype(np.int64))
            vals.append(K.data)
            continue
        if kind == "edge_spring":
            K = np.broadcast_to(0.5 * wi * np.array([[1.0, -1.0], [-1.0, 1.0]]), (n, 2, 2))
        elif kind == "tris_strain":
            D = q["DmInv"]
            G = np.concatenate([D, -D.sum(axis=2)[:, :, None]], axis=2)             # (n, 2, 3)
            K = np.einsum("nja,njb->nab", G, G) * (wi * np.abs(q["A0"]))[:, None, None]
        else:
            D = q["DmInv"]
            G = np.concatenate([D, -D.sum(axis=1)[:, None, :]], axis=1)             # (n, 4, 3)
            K = np.einsum("nac,nbc->nab", G, G) * (wi * np.abs(q["V0"]))[:, None, None]
        nv = setup.width
        rows.append(np.broadcast_to(idx[:, :, None], (n, nv, nv)).reshape(-1))
        cols.append(np.broadcast_to(idx[:, None, :], (n, nv, nv)).reshape(-1))
        vals.append(np.ascontiguousarray(K).reshape(-1))
    A = sparse.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n_verts, n_verts)).tocsr()
    A = ((A + A.T) * 0.5).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


SlabPlan = collections.namedtuple("SlabPlan", "order slab_ptr A_perm")
SLAB_TARGET = 256           # the default slab size of the global step's slab solver (within 16 % of the best of
                            # {64, 128, 256, 512, 1536} at both measured shapes; the geodesics' 1536 is 2.3x slower at N = 4 096)


def slab_plan(A, target=SLAB_TARGET):
    """The slab plan of the global step's block-tridiagonal solver (csrc/asb_gslab.hip) for the system matrix ``A`` (scipy CSR,
    symmetric pattern): ``geodesic.bfs_slabs`` on A's own graph -- the mesh graph, or its square for ``verts_bending`` -- groups
    breadth-first level sets into slabs of at least ``target`` vertices.  Returns ``SlabPlan(order, slab_ptr, A_perm)``:
    ``order`` (N,) permuted index -> vertex, ``slab_ptr`` (slabs + 1,) the slab boundaries in the permuted numbering and
    ``A_perm`` = A[order][:, order] as CSR with sorted indices.  Disconnected meshes give their components as further slabs;
    a ``target`` of N or more gives one slab.  The plan is VERIFIED: an entry of ``A_perm`` that couples slabs more than one
    apart raises ValueError -- a silent violation would give wrong positions."""
    from scipy import sparse
    from .geodesic import bfs_slabs
    if not sparse.issparse(A) or A.shape[0] != A.shape[1] or A.shape[0] < 1:
        raise ValueError("slab_plan: a square sparse matrix expected")
    try:
        t = int(target)
    except (TypeError, ValueError):
        t = 0
    if t != target or isinstance(target, bool) or t < 1:
        raise ValueError("slab_plan: target %r: a positive number of vertices per slab" % (target,))
    A = sparse.csr_matrix(A)
    order, ptr = bfs_slabs(A, t)
    order = np.ascontiguousarray(order, dtype=np.int64)
    ptr = np.ascontiguousarray(ptr, dtype=np.int64)
    Ap = A[order][:, order].tocsr()
    Ap.sort_indices()
    check_slab_plan(Ap, ptr)
    return SlabPlan(order, ptr, Ap)


def check_slab_plan(A_perm, slab_ptr):
    """Raises ValueError unless the slabs cover 0 .. N in ascending order and no entry of the permuted CSR ``A_perm`` couples
    slabs more than one apart."""
    n = A_perm.shape[0]
    ptr = np.asarray(slab_ptr, dtype=np.int64)
    if ptr.ndim != 1 or ptr.size < 2 or ptr[0] != 0 or ptr[-1] != n or (np.diff(ptr) < 1).any():
        raise ValueError("slab_plan: the slabs %r do not cover 0 .. %d in ascending order" % (ptr.tolist()[:8], n))
    slab = np.searchsorted(ptr, np.arange(n), side="right") - 1
    rows = np.repeat(np.arange(n), np.diff(A_perm.indptr))
    far = np.abs(slab[rows] - slab[A_perm.indices]) > 1
    if far.any():
        e = int(np.flatnonzero(far)[0])
        raise ValueError("slab_plan: entry (%d, %d) of the permuted matrix couples slabs %d and %d: not block tridiagonal"
                         % (rows[e], A_perm.indices[e], slab[rows[e]], slab[A_perm.indices[e]]))


SUBSPACE_MAX_R = 8192       # the engine's limit of a position subspace (GB_MAX_R of csrc/asb_gsub.hip): three dense r x r inverses


def subspace_basis(basis, num_components=None, n_verts=None):
    """The host preparation of the global step's position subspace q = o + U z (csrc/asb_gsub.hip): per coordinate d a thin
    Euclidean QR of U_d = comps[:r, :, d].T (N x r); returns ``Qt`` (3, r, N) float64 with Qt[d] = Q_d^T.  Q_d spans what U_d
    spans, so the Galerkin projection is the same, and kappa(Q_d^T A Q_d) <= kappa(A).

    ``basis``: a world-space array (K, N, 3), the path of a ``.npy`` holding one, or a ``posComponents`` -- its ``comps``,
    multiplied by its snapshots' ``invMassL`` where they live in the mass-weighted space (snapshots with masses, unless
    ``post_process_components`` has run with ``q_massWeight`` and taken them back: the class's ``_comps_post_processed``
    says so); scale does not matter, only the span.  ``num_components`` = r: the first
    r components, None: all K.  ``n_verts``: the N the basis must have (None: not checked).  The input is left untouched.
    ValueError: a wrong shape, r outside 1 .. K, r > N, entries that are not finite, and a rank-deficient U_d, named by its
    coordinate -- min |R_ii| <= N eps max |R_ii| (the convention of ``numpy.linalg.matrix_rank``)."""
    if isinstance(basis, (str, bytes)) or hasattr(basis, "__fspath__"):
        try:
            comps = np.load(basis)
        except (OSError, ValueError) as e:
            raise ValueError("subspace_basis: no array could be read from %r (%s)" % (basis, e))
    elif hasattr(basis, "comps"):
        comps = np.asarray(basis.comps, dtype=np.float64)
        snaps = getattr(basis, "pos_snapshots", None)
        inv = getattr(snaps, "invMassL", None)
        # un-weighted already only where post_process_components HAS run with q_massWeight (the class's own flag says whether)
        done = bool(getattr(basis, "_comps_post_processed", False)) and bool(getattr(getattr(basis, "param", None), "q_massWeight", False))
        if inv is not None and comps.ndim == 3 and not done:
            comps = comps * np.asarray(inv, dtype=np.float64)[None, :, None]
    else:
        comps = basis
    try:
        comps = np.asarray(comps, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("subspace_basis: the basis is no numeric array")
    if comps.ndim != 3 or comps.shape[2] != 3 or comps.shape[0] < 1 or comps.shape[1] < 1:
        raise ValueError("subspace_basis: a basis of shape %s: (K, N, 3) expected" % (comps.shape,))
    K, N = comps.shape[:2]
    if n_verts is not None and N != n_verts:
        raise ValueError("subspace_basis: the basis has %d vertices, the snapshots %d" % (N, n_verts))
    r = K if num_components is None else num_components
    if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 1 <= r <= K:
        raise ValueError("subspace_basis: num_components %r: an integer 1 .. %d (the basis' components) or None" % (num_components, K))
    r = int(r)
    if r > N:
        raise ValueError("subspace_basis: %d components for %d vertices: at most N per coordinate" % (r, N))
    if not np.isfinite(comps[:r]).all():
        raise ValueError("subspace_basis: the basis holds entries that are not finite")
    Qt = np.empty((3, r, N))
    for d in range(3):
        Q, R = np.linalg.qr(comps[:r, :, d].T)
        diag = np.abs(np.diag(R))
        if diag.min() <= N * np.finfo(np.float64).eps * diag.max():
            raise ValueError("subspace_basis: the first %d components are rank deficient in coordinate %s (min |R_ii| = %.3g, max %.3g)"
                             % (r, "xyz"[d], diag.min(), diag.max()))
        Qt[d] = Q.T
    return Qt


def project_host(setup, positions, sigma_min=1.0, sigma_max=1.0):
    """NumPy restatement of ``get_pi`` for every element and frame: positions (F, N, 3) -> (F, n p, 3).  For scale and for
    checks on small shapes only; the product path is the device kernel."""
    X = np.asarray(positions, dtype=np.float64)
    F = X.shape[0]
    idx, kind, q = setup.idx, setup.kind, setup.parts
    if kind == "edge_spring":                                        # (:297-311): 0.5 (pi2 - pi1) = 0.5 d s / |s|
        s = X[:, idx[:, 1]] - X[:, idx[:, 0]]
        ln = np.linalg.norm(s, axis=2)
        with np.errstate(divide="ignore", invalid="ignore"):
            return 0.5 * q["d"][None, :, None] * s / ln[..., None]
    if kind == "tris_strain":                                        # (:411-425)
        Ds = np.stack([X[:, idx[:, 1]] - X[:, idx[:, 0]], X[:, idx[:, 2]] - X[:, idx[:, 0]]], axis=3)
        Fm = np.einsum("tij,ftik->ftjk", q["P"], Ds) @ q["DmInv"][None]
        U, s, Vt = np.linalg.svd(Fm)
        Fh = (U * np.clip(s, sigma_min, sigma_max)[..., None, :]) @ Vt
        pi = np.swapaxes(np.einsum("tij,ftjk->ftik", q["P"], Fh), 2, 3)
        return pi.reshape(F, -1, 3)
    if kind in ("tets_strain", "tets_deformation_gradient"):         # (:538-554, :673-687)
        x4 = X[:, idx[:, 3]]
        Ds = np.stack([X[:, idx[:, 0]] - x4, X[:, idx[:, 1]] - x4, X[:, idx[:, 2]] - x4], axis=3)
        Fm = Ds @ q["DmInv"][None]
        U, s, Vt = np.linalg.svd(Fm)
        if kind == "tets_strain":
            s = np.clip(s, sigma_min, sigma_max)
            s[..., 2] = np.where(np.linalg.det(Fm) < 0.0, -s[..., 2], s[..., 2])
            return ((U * s[..., None, :]) @ Vt).reshape(F, -1, 3)
        R = U @ Vt
        R[..., 2] = np.where((np.linalg.det(R) < 0)[..., None], -R[..., 2], R[..., 2])
        return np.swapaxes(R, 2, 3).reshape(F, -1, 3)
    out = np.empty((F, setup.n_elem, 3))                            # verts_bending (:199-215)
    ptr, v2, w = q["star_ptr"], q["star_idx"], q["weights"]
    for i, v in enumerate(q["indices"]):
        ss = np.zeros((F, 3))
        for e in range(ptr[i], ptr[i + 1]):
            ss += (X[:, v] - X[:, v2[e]]) * w[e]
        nrm = np.linalg.norm(ss, axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            corr = np.where((nrm < 1e-10)[:, None], q["normal"][i][None] * q["rest_curvature"][i],
                            ss * (q["rest_curvature"][i] / nrm)[:, None])
        flip = (nrm > 1e-5) & ((corr @ q["normal"][i]) * q["dot_with_normal"][i] < 0)
        out[:, i] = np.where(flip[:, None], -corr, corr)
    return out
