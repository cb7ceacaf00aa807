"""GPU (-m gpu): the constraint projections on flat, collapsed, inverted and badly scaled elements -- the device probe
asb_test_cproj_project_dev and the real kernels k_cproj (posSnapshots.constraint_projections) and k_cproj_em
(engine.cforce_run) of csrc/asb_cproj.hip -- against the 60-digit model of tests/cproj_model.py on the families of
tests/cproj_cases.py, with the bars of tests/test_cproj_model_cpu.py (8 x LAPACK's worst, floored at 16); and cp_bend / cp_edge
at their thresholds against a numpy.longdouble restatement.

The real kernels get F prescribed exactly: element e is a rest tet with corners e_1, e_2, e_3, 0 (DmInv = I exactly), the frame
puts corner 4 on the origin and corners 1 .. 3 on the columns of F, and the raw tensor holds them bit for bit; for tris_strain
the rest triangle is 0, e_1, e_2 (P = [e_1 e_2], DmInv = I).  The cases at the scales 2^-27, 1, 2^27 are laid out over
17 elements x 65 frames -- one element past the 16-element block, one frame past the 64-frame tile, every family in both edge
lanes -- and one call per distinct clamp projects the whole layout; the cases that own the clamp are checked against the
model, and every matrix against its copies elsewhere in the layout, bit for bit.  The extreme scales stay with the probes."""
import contextlib
import io

import numpy as np
import pytest

import cproj_cases as cc
import cproj_model as cm
from conftest import load_golden

pytestmark = pytest.mark.gpu

EPS = cm.EPS
LD = np.longdouble
NE, NF = 17, 65


@pytest.fixture(scope="module")
def model():
    """n -> list of dict(fam, label, F, lo, hi, dec, exp (kind -> expected)), the 60-digit references once per module"""
    out = {}
    for n in (2, 3):
        kinds = [k for k, d in cc.DIM.items() if d == n]
        out[n] = []
        for fam, label, F, lo, hi in cc.all_cases(n):
            dec = cm.decompose(F)
            out[n].append(dict(fam=fam, label=label, F=F, lo=lo, hi=hi, dec=dec, exp={k: cm.expected(dec, k, lo, hi) for k in kinds}))
    return out


def _snaps(frames):
    from animsnapbases_amd import posSnapshots
    with contextlib.redirect_stdout(io.StringIO()):
        return posSnapshots.from_arrays(np.array(frames), None, "first", standarize=False, massWeight=False)


def _by_clamp(cases):
    groups = {}
    for c in cases:
        groups.setdefault((c["lo"], c["hi"]), []).append(c)
    return groups


# ------------------------------------------------------------------ 1. the device probe
def _normalised_gap(kind, c, a, b):
    """max|a - b| in the units of the kind's unique-result measure"""
    s, exp = c["dec"]["s"], c["exp"][kind]
    d = np.abs(np.asarray(a) - np.asarray(b)).max()
    if kind == "tets_deformation_gradient":
        return d * float((s[1] + s[2]) / (2 * s[0])) / EPS
    return d / float(exp["kappa"] * max(exp["c"][0], s[0])) / EPS


@pytest.mark.parametrize("kind", ("tets_strain", "tets_deformation_gradient", "tris_strain"))
def test_device_probe_against_60_digit_model(model, kind):
    """every family and scale on the device, one thread per matrix, against the bars of the CPU test; host and device within the
    sum of the two bars of each other wherever the result is unique (contraction differs between the two builds, so no bit
    equality; with two vanished singular values the complement of u_1 may legitimately differ)"""
    from animsnapbases_amd import HipEngine
    eng = HipEngine(0)
    n = cc.DIM[kind]
    worst, gap, checked = {}, {}, 0
    for (lo, hi), group in _by_clamp(model[n]).items():
        dev = eng.test_cproj_project_dev(cm.KINDS[kind], np.array([c["F"] for c in group]), lo, hi)
        assert dev.shape == (len(group), n, n)
        for c, out in zip(group, dev):
            m = cc.check_case(kind, c["fam"], c["label"], c["F"], lo, hi, out, c["dec"], c["exp"][kind], "device probe")
            checked += 1
            w = worst.setdefault(c["fam"], {})
            for key in cm.MEASURES:
                if m[key] is not None:
                    w[key] = max(w.get(key, 0.0), m[key])
            host = cc.host_probe(kind, c["F"], lo, hi)
            if c["dec"]["rank"] == 0:
                assert np.array_equal(host, out), c["label"]
            elif c["exp"][kind]["ref"] is not None:
                key = "rot" if kind == "tets_deformation_gradient" else "err"
                g = _normalised_gap(kind, c, host, out)
                gap[c["fam"]] = max(gap.get(c["fam"], 0.0), g)
                assert g <= 2 * cc.bounds(kind, c["fam"])[key], (c["label"], g)
    assert checked == len(model[n])                 # no case skipped
    for fam in sorted(worst):
        b = cc.bounds(kind, fam) if fam != "zero" else {}
        print("device probe %s %-9s" % (kind, fam), " ".join("%s=%.3g/%.3g" % (k, v, b[k]) for k, v in sorted(worst[fam].items()) if k in b),
              "host-device %.3g" % gap.get(fam, 0.0))


# ------------------------------------------------------------------ 2. the real kernels
def _layout(cases):
    """slot (e, f) -> case index: frame 64, element 16 and the interior are each filled with the cases taken round-robin over the
    families, so that every family has a copy in both edge lanes and in the interior; every case occurs, most several times"""
    fams = {}
    for i, c in enumerate(cases):
        fams.setdefault(c["fam"], []).append(i)
    order, depth = [], 0
    while len(order) < len(cases):
        order += [idx[depth] for idx in fams.values() if depth < len(idx)]
        depth += 1
    lanes = ([(e, NF - 1) for e in range(NE)], [(NE - 1, f) for f in range(NF - 1)],
             [(e, f) for f in range(NF - 1) for e in range(NE - 1)])
    assert sum(len(x) for x in lanes) == NE * NF and len(lanes[2]) >= len(cases)
    where = np.empty((NE, NF), dtype=np.int64)
    for lane in lanes:                              # each lane starts the round over: one of every family first
        for j, (e, f) in enumerate(lane):
            where[e, f] = order[j % len(order)]
    for fam, idx in fams.items():
        own = np.isin(where, idx)
        assert own[NE - 1].any() and own[:, NF - 1].any() and own[:NE - 1, :NF - 1].any(), fam
    assert len(np.unique(where)) == len(cases)
    return where


def _mesh(n, cases, where):
    """rest positions, elements, frames (NF, N, 3) that put the layout's F into every (element, frame), the selection CSR that
    copies the projections into the force tensor, and the vertex rows it fills"""
    from scipy import sparse
    nv, p = n + 1, n
    rest = np.zeros((NE * nv, 3))
    frames = np.zeros((NF, NE * nv, 3))
    el = np.arange(NE * nv).reshape(NE, nv)
    for e in range(NE):
        if n == 3:                                  # corners e_1, e_2, e_3, 0
            rest[nv * e:nv * e + 3] = np.eye(3)
        else:                                       # corners 0, e_1, e_2
            rest[nv * e + 1:nv * e + 3, :2] = np.eye(2)
        for f in range(NF):
            F = cases[where[e, f]]["F"]
            if n == 3:
                frames[f, nv * e:nv * e + 3] = F.T                      # corner j = column j
            else:
                frames[f, nv * e + 1:nv * e + 3, :2] = F.T
                frames[f, nv * e + 1:nv * e + 3, 2] = (0.25, -0.5)      # out of the rest plane: P takes no part of it
    rows = np.array([nv * e + (i if n == 3 else i + 1) for e in range(NE) for i in range(p)])
    St = sparse.csr_matrix((np.ones(NE * p), (rows, np.arange(NE * p))), shape=(NE * nv, NE * p))
    St.sort_indices()
    return rest, el, frames, St, rows


def _oriented(n, block):
    """(NF, NE p, 3) -> (NF, NE, n, n) in the probes' orientation"""
    if n == 3:
        return block.reshape(NF, NE, 3, 3)
    b = block.reshape(NF, NE, 2, 3)
    assert (b[..., 2] == 0.0).all()                 # (P Fhat)^T with P = [e_1 e_2]: no z
    return np.swapaxes(b[..., :2], 2, 3)            # rows of (P Fhat)^T are the columns of Fhat


@pytest.mark.parametrize("n", (3, 2))
def test_kernels_on_prescribed_deformation_gradients(model, n):
    import torch
    from animsnapbases_amd import projections as proj
    lg2 = {int(np.log2(k)) for k in cc.KERNEL_SCALES}
    cases = [c for c in model[n] if c["fam"] == "zero" or int(c["label"].rsplit("^", 1)[1]) in lg2]
    assert len(cases) == (len(model[n]) - 2) // 2 + 2
    where = _layout(cases)
    rest, el, frames, St, rows = _mesh(n, cases, where)
    kinds = [k for k, d in cc.DIM.items() if d == n]
    setups = {k: proj.build_setup(k, el, rest) for k in kinds}
    for k in kinds:                                 # F is the frame's corner differences, exactly
        assert np.array_equal(setups[k].parts["DmInv"], np.broadcast_to(np.eye(n), (NE, n, n)))
        if n == 2:
            assert np.array_equal(setups[k].parts["P"], np.broadcast_to(np.eye(3)[:, :2], (NE, 3, 2)))
    snaps = _snaps(frames)
    eng = snaps._engine
    first = {id(c): tuple(np.argwhere(where == i)[0]) for i, c in enumerate(cases)}
    e0 = np.array([[first[id(cases[where[e, f]])][0] for e in range(NE)] for f in range(NF)])         # (NF, NE): the first copy
    f0 = np.array([[first[id(cases[where[e, f]])][1] for e in range(NE)] for f in range(NF)])
    assert ((e0 != np.arange(NE)[None]) | (f0 != np.arange(NF)[:, None])).sum() >= NE * NF // 2
    worst, checked = {}, {k: 0 for k in kinds}
    for (lo, hi), group in _by_clamp(cases).items():
        for kind in kinds:
            out, nF, nrows = snaps.constraint_projections(kind, el, rest_positions=rest, sigma_min=lo, sigma_max=hi)
            assert (nF, nrows) == (NF, NE * n)
            buf = torch.full((NF, rest.shape[0], 3), float("nan"), dtype=torch.float64, device=out.device)
            torch.cuda.synchronize()                # the fill is on torch's stream, the kernels on the engine's own
            eng.cproj_setup(setups[kind])
            eng.cforce_run(0, 0, NF, 1, None, False, 1.0, lo, hi, St, False, 0, buf.data_ptr())
            force = buf.cpu().numpy()
            assert (np.delete(force, rows, axis=1) == 0.0).all()       # the empty rows of the selection
            for who, block in (("k_cproj", out.cpu().numpy()), ("k_cproj_em", force[:, rows])):
                got = _oriented(n, block)
                # a neighbour of a deficient element comes out as it does alone: every copy of a matrix, wherever it lies
                assert np.array_equal(got, got[f0, e0]), (who, kind, lo, hi)
                for c in group:
                    e, f = first[id(c)]
                    m = cc.check_case(kind, c["fam"], c["label"], c["F"], lo, hi, got[f, e], c["dec"], c["exp"][kind], who)
                    w = worst.setdefault((who, kind, c["fam"]), {})
                    for key in cm.MEASURES:
                        if m[key] is not None:
                            w[key] = max(w.get(key, 0.0), m[key])
            checked[kind] += len(group)
    assert all(v == len(cases) for v in checked.values())              # no case skipped
    for (who, kind, fam) in sorted(worst):
        b = cc.bounds(kind, fam) if fam != "zero" else {}
        print("%-10s %s %-9s" % (who, kind, fam), " ".join("%s=%.3g/%.3g" % (k, v, b[k]) for k, v in sorted(worst[(who, kind, fam)].items()) if k in b))


# ------------------------------------------------------------------ 3. cp_bend at its thresholds
def _bend_ld(q, X):
    """numpy.longdouble restatement of Constraint_projections.py:199-215 on float64 positions X (N, 3) with the rest tables q:
    -> ss (n, 3), |terms| (n, 3), nrm (n), result (n, 3), flipped (n), the product dot * dot_with_normal (n)"""
    ptr, v2, w = q["star_ptr"], q["star_idx"], q["weights"].astype(LD)
    n = len(q["indices"])
    ss, tt, res = np.zeros((n, 3), dtype=LD), np.zeros((n, 3), dtype=LD), np.zeros((n, 3), dtype=LD)
    nrm, flip, prod = np.zeros(n, dtype=LD), np.zeros(n, dtype=bool), np.zeros(n, dtype=LD)
    X = X.astype(LD)
    for i, v in enumerate(q["indices"]):
        for e in range(ptr[i], ptr[i + 1]):
            d = (X[v] - X[v2[e]]) * w[e]
            ss[i] += d
            tt[i] += np.abs(d)
        nrm[i] = np.sqrt((ss[i] * ss[i]).sum())
        rmc, nor = LD(q["rest_curvature"][i]), q["normal"][i].astype(LD)
        res[i] = nor * rmc if nrm[i] < 1e-10 else ss[i] * (rmc / nrm[i])
        prod[i] = (res[i] * nor).sum() * LD(q["dot_with_normal"][i])
        flip[i] = nrm[i] > 1e-5 and prod[i] < 0
        if flip[i]:
            res[i] = -res[i]
    return ss, tt, nrm, res, flip, prod


def test_bending_at_its_three_branches():
    """cp_bend on the rest tables of the open grid: the whole star on one point (ss = 0 exactly: normal x rest curvature, no flip);
    the rest pose shrunk about a vertex by 1e-12 (nrm < 1e-11: the same branch), by 1e-8 and 1e-7 (1e-9 <= nrm <= 1e-6, but for
    four vertices at 1e-8, which stay above 4e-10: the direction of ss, and no flip even where it is opposed -- the mirrored
    copies); the rest pose mirrored through a tangent plane
    (nrm > 1e-5 and opposed: flipped).  Which branch a frame takes is asserted from the longdouble restatement, a factor 10
    away from either threshold (a factor 4 for those four); the device within 64 eps of the restatement's terms: rest curvature x sum |w (x - y)| / nrm."""
    from animsnapbases_amd import projections as proj
    g = load_golden("cproj_verts_bending_grid")
    rest, tris = g["rest"], g["elements"]
    q = proj.build_setup("verts_bending", tris, rest).parts
    for key in ("weights", "rest_curvature", "normal", "dot_with_normal"):
        assert np.allclose(q[key], g[key], rtol=1e-12, atol=1e-14), key        # the reference's tables, to rounding
    v0 = int(q["indices"][len(q["indices"]) // 2])
    c, nor = rest[v0], q["normal"][len(q["indices"]) // 2]
    H = np.eye(3) - 2.0 * np.outer(nor, nor) / (nor @ nor)
    shrunk = {s: c + s * (rest - c) for s in (1e-12, 1e-8, 1e-7)}
    frames = [rest, np.broadcast_to(np.array([0.3, -0.2, 0.7]), rest.shape)]
    frames += [shrunk[s] for s in (1e-12, 1e-8, 1e-7)]
    frames += [c + (shrunk[s] - c) @ H.T for s in (1e-8, 1e-7)]
    frames.append(c + (rest - c) @ H.T)
    frames = np.array(frames)
    snaps = _snaps(frames)
    snaps.tris = tris
    out, nF, nrows = snaps.constraint_projections("verts_bending", tris, rest_positions=rest)
    out = out.cpu().numpy()
    assert (nF, nrows) == (len(frames), len(q["indices"]))
    worst = 0.0
    for f, X in enumerate(frames):
        ss, tt, nrm, res, flip, prod = _bend_ld(q, X)
        if f == 1:
            assert (ss == 0).all() and not flip.any()
        elif f == 2:
            assert (nrm < 1e-11).all() and (nrm > 0).all() and not flip.any()
        elif f in (3, 4, 5, 6):
            assert (nrm <= 1e-6).all() and not flip.any()
            if f in (4, 6):
                assert (nrm >= 1e-9).all()
            else:                                   # 1e-8 x the four flattest vertices' rest curvature (0.043 .. 0.098) is 4.3e-10 ..
                assert (nrm >= 1e-9).sum() >= 16 and (nrm >= 4e-10).all()          # 9.8e-10: a factor 4, not 10, above 1e-10
            if f >= 5:
                assert (prod < 0).sum() >= len(nrm) // 2           # opposed, and still not flipped
        else:
            assert (nrm >= 1e-4).all()
            if f == 7:
                assert flip.sum() >= len(nrm) // 2
        rmc = q["rest_curvature"].astype(LD)
        small = nrm < 1e-10
        tol = np.where(small[:, None], np.abs(q["normal"]) * rmc[:, None],
                       rmc[:, None] * np.sqrt((tt * tt).sum(axis=1))[:, None] / np.where(small, 1, nrm)[:, None]) * 64 * EPS
        # no flip decision within rounding of zero
        decided = nrm > 1e-5
        assert (np.abs(prod[decided]) > 1e3 * EPS * np.abs(q["dot_with_normal"][decided]) * rmc[decided]).all()
        err = np.abs(out[f].astype(LD) - res)
        assert np.isfinite(out[f]).all()
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), (f, float((err / tol).max()))
        if f in (1, 2):                             # one product, one rounding
            assert np.array_equal(out[f], q["normal"] * q["rest_curvature"][:, None])
    print("verts_bending: worst error / (64 eps terms) %.3g" % worst)


# ------------------------------------------------------------------ 4. cp_edge: a tiny edge next to a collapsed one
def test_tiny_edge_and_collapsed_edge():
    """an edge of length 5 x 2^-500, whose squared length 25 x 2^-1000 is still a normal number: the direction is right, not NaN;
    the exactly collapsed edge next to it is NaN in its three entries and nowhere else"""
    t = 2.0 ** -500
    rest = np.array([[0.0, 0, 0], [1.0, 0, 0], [1.0, 1, 0], [0.0, 1, 0], [0.0, 0, 1]])
    edges = np.array([[4, 2], [0, 1], [2, 3], [0, 4], [3, 4]])
    frame = np.array([[0.0, 0, 0], [3 * t, -4 * t, 0], [0.5, 0.25, -1.0], [0.5, 0.25, -1.0], [0.0, 2.0, 0.0]])
    frames = np.array([rest, frame, frame])
    snaps = _snaps(frames)
    out = snaps.constraint_projections("edge_spring", edges, rest_positions=rest)[0].cpu().numpy()
    d = np.linalg.norm(rest[edges[:, 1]] - rest[edges[:, 0]], axis=1).astype(LD)
    s = (frame[edges[:, 1]] - frame[edges[:, 0]]).astype(LD)
    ln = np.sqrt((s * s).sum(axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        want = 0.5 * d[:, None] * s / ln[:, None]
    assert ln[1] == 5 * LD(t) and ln[2] == 0
    for f in (1, 2):
        assert np.array_equal(np.isnan(out[f]), np.isnan(want)) and np.isnan(out[f]).sum() == 3 and np.isnan(out[f][2]).all()
        ok = ~np.isnan(want)
        # |s|^2, its root, 0.5 d / |s| and the product: five roundings at the most
        assert (np.abs(out[f][ok].astype(LD) - want[ok]) <= 8 * EPS * 0.5 * np.broadcast_to(d[:, None], want.shape)[ok]).all()
    assert np.abs(out[1][1] - np.array([0.3, -0.4, 0.0])).max() <= 4 * EPS
