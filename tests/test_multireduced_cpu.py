"""CPU: the host side of several reduced constraint kinds in one solve (``posSnapshots.set_reduced_kinds``) --
``projections.touched_setup(into=)`` / ``touched_union`` (every kind's sampled elements numbered in ONE ascending vertex list) on
the five element kinds, the multi-kind affine form c + sum_k G_k coef_k of tests/multireduced_cases.py against its multi-kind
host model, the coverage the strip fixtures of the GPU tests are chosen for, and the refusals and engine-call sequences of
``solve_frames`` / ``simulate_frames`` on a recording double of the engine."""
import numpy as np
import pytest

from conftest import load_golden
import multireduced_cases as mc
from pdsolve_cases import KS, MODES, bound_K, explicit_state
from test_dynamics_trace_cpu import RecordingEngine, _bare, _inputs, _kinds

from animsnapbases_amd import _lib, projections as proj

FIVE = ["edge_spring", "tris_strain", "tets_strain", "tets_deformation_gradient", "verts_bending_closed"]


def _kind(name):
    return "verts_bending" if name.startswith("verts_bending") else name


# ------------------------------------------------------------------ 1. a set-up renumbered into a given vertex list
@pytest.mark.parametrize("name", FIVE)
def test_renumbering_into_a_given_list_is_bit_identical(name):
    g = load_golden("cproj_" + name)
    full = proj.build_setup(_kind(name), g["elements"], g["rest"])
    N = g["rest"].shape[0]
    rng = np.random.default_rng(11)
    q = np.array(g["frames"][:7])
    subs = [proj.subset_setup(full, sel) for sel in (np.array([0]), rng.choice(full.n_elem, size=min(5, full.n_elem), replace=False),
                                                    np.array([full.n_elem - 1, 0, full.n_elem - 1]))]
    own = [proj.touched_setup(s)[0] for s in subs]
    union = proj.touched_union(subs)
    assert union.dtype == np.int64 and union.tolist() == sorted(set(np.concatenate(own).tolist()))          # sorted and unique
    extra = np.setdiff1d(np.arange(N), union)
    lists = [union, np.arange(N, dtype=np.int64)] + ([np.sort(np.concatenate([union, extra[:2]]))] if extra.size else [])
    for sub, mine in zip(subs, own):
        a = proj.project_host(sub, q, *g["sigma"])
        # today's calls keep their results: into=own touched set is touched_setup(sub) itself
        t0, c0 = proj.touched_setup(sub)
        t1, c1 = proj.touched_setup(sub, into=mine)
        assert np.array_equal(t0, t1) and np.array_equal(c0.idx, c1.idx)
        for into in lists:
            touched, compact = proj.touched_setup(sub, into=into)
            assert np.array_equal(touched, into) and touched.dtype == np.int64
            assert compact.idx.max() < into.shape[0] and np.array_equal(into[compact.idx], sub.idx)     # positions in the list
            assert compact.table is sub.table or np.array_equal(compact.table, sub.table)
            if sub.star_idx is not None:
                assert np.array_equal(into[compact.star_idx], sub.star_idx) and np.array_equal(compact.star_ptr, sub.star_ptr)
                assert np.array_equal(compact.bending_indices, sub.bending_indices)
            assert np.array_equal(proj.project_host(compact, q[:, into], *g["sigma"]), a)                # bit for bit
    big = max(range(len(subs)), key=lambda i: own[i].shape[0])
    with pytest.raises(ValueError, match="lacks"):
        proj.touched_setup(subs[big], into=own[big][:-1] if own[big].shape[0] > 1 else own[big] + 1)
    with pytest.raises(ValueError, match="ascending"):
        proj.touched_setup(subs[big], into=np.concatenate([own[big], own[big][-1:]]))
    with pytest.raises(ValueError, match="either"):
        proj.touched_setup(subs[big], N, into=union)


# ------------------------------------------------------------------ 2. the fixtures are what the GPU tests need them to be
def test_strip_cases_cover_the_row_counts():
    """Union sizes below, at and above the 32-vertex tile, ragged ones, N_t = N, unions larger than either kind's own set; every
    normal matrix within ``COND_CAP`` (``strip_case`` asserts it per operator)."""
    sizes, whole, larger = set(), set(), 0
    for n in mc.STRIPS:
        c = mc.strip_case(n)
        assert c["ms"][0] and c["ms"][0][0] == 1 and c["ms"][1][0] == 1 and c["kappa"] <= 40.0
        for me, mt in mc.strip_pairs(c):
            ops = {0: c["op"](0, me), 1: c["op"](1, mt)}
            assert max(o.cond.max() for o in ops.values()) <= mc.COND_CAP
            union, compact, own = mc.sampled(c, ops)
            assert union.tolist() == sorted(set(own[0].tolist()) | set(own[1].tolist()))
            sizes.add(int(union.shape[0]))
            if union.shape[0] == n:
                whole.add(n)
            larger += union.shape[0] > max(own[0].shape[0], own[1].shape[0])
    assert min(sizes) == 3 and max(sizes) == 60 and {32, 33} <= sizes and any(s < 32 for s in sizes)
    assert {3, 31, 32, 33} <= whole and larger >= 10
    c = mc.strip_case(15)
    union, _, own = mc.sampled(c, {0: c["op"](0, 1), 1: c["op"](1, 1)})
    assert (own[0].shape[0], own[1].shape[0], union.shape[0]) == (4, 6, 7)
    # the pairs of the GPU test exist where a strip is long enough, with contraction lengths 4 + 4, 4 + 20 and 20 + 4
    assert mc.strip_pairs(mc.strip_case(65), mc.STRIP_PAIRS) == mc.STRIP_PAIRS and mc.strip_pairs(mc.strip_case(3), mc.STRIP_PAIRS) == [(1, 1)]


def test_fixture_a_is_what_the_golden_was_generated_from():
    a = mc.combined_case()
    z = mc.golden_combined()
    assert z["edge_ms"].tolist() == list(mc.EDGE_MS) and z["tet_ms"].tolist() == list(mc.TET_MS) and z["mixed_ms"].tolist() == list(mc.MIXED_MS)
    assert a["frames"].shape == (130, 18, 3) and [k[0].n_elem for k in a["kinds"]] == [68, 68]
    # the stored edge basis is orthonormal per coordinate and its points are rows of the 68 edges
    for d in range(3):
        C = z["edge_components"][:, :, d]
        assert np.abs(C @ C.T - np.eye(C.shape[0])).max() < 1e-12
    assert z["edge_components"].shape == (17, 68, 3) and 0 <= z["edge_Pt"].min() and z["edge_Pt"].max() < 68
    sizes = set()
    for me in mc.EDGE_MS:
        for mt in mc.TET_MS:
            ops = {0: a["op"](0, me), 1: a["op"](1, mt)}
            assert max(o.cond.max() for o in ops.values()) <= mc.COND_CAP
            sizes.add(int(mc.sampled(a, ops)[0].shape[0]))
            for mode in MODES:
                assert all(float(z[mc.amp_key(me, mt, mode, K)]) <= mc.AMP_CAP for K in KS)
    assert min(sizes) == 8 and max(sizes) == 18


# ------------------------------------------------------------------ 3. the affine form against the host model
@pytest.mark.parametrize("pair", [(1, 17), (17, 1), (4, 17), (3, 1)])
def test_affine_form_matches_the_multi_kind_host_model(pair):
    a = mc.combined_case()
    z = mc.golden_combined()
    F = a["frames"].shape[0]
    ops = {0: a["op"](0, pair[0]), 1: a["op"](1, pair[1])}
    for mode in MODES:
        host = mc.model(a, range(F), mode, KS, reduced=ops)
        parts = mc.affine_parts(a, ops, range(F), mode)
        q = explicit_state(a["frames"], range(F), mode)
        for k in range(1, max(KS) + 1):
            q = mc.affine_step(a, ops, q, parts)
            if k in KS:
                B = bound_K(mc.one_bound(a, ops, a["frames"], True), k, float(z[mc.amp_key(pair[0], pair[1], mode, k)]))
                err = np.abs(q - host[k]).max()
                print("me = %d mt = %d %s K = %d: err %.3g, B_K %.3g, err / B_K %.3g" % (pair + (mode, k, err, B, err / B)))
                assert err <= B
        # not vacuous: reducing the edges as well moves the result by far more than the bound
        tets_only = mc.model(a, range(F), mode, (10,), reduced={1: ops[1]})[10]
        assert np.abs(host[10] - tets_only).max() > 1e3 * B


def test_affine_form_on_a_strip():
    """One iteration of the affine form on the union against A^-1 (ms + sum_k S_k^T V_k H_k p_k) by SciPy's solve."""
    for n in (3, 17, 65):
        c = mc.strip_case(n)
        sel = list(range(0, 130, 7))
        for me, mt in mc.strip_pairs(c, mc.STRIP_PAIRS):
            ops = {0: c["op"](0, me), 1: c["op"](1, mt)}
            q = explicit_state(c["frames"], sel, "difference")
            want = mc.model(c, sel, "difference", (1,), reduced=ops)[1]
            got = mc.affine_step(c, ops, q, mc.affine_parts(c, ops, sel, "difference"))
            P = {i: v[1] for i, v in mc.coefficients(c, ops, q).items()}
            assert np.abs(got - want).max() <= mc.one_bound(c, ops, q, True, P)


# ------------------------------------------------------------------ 4. the public methods on a recording engine
def _patched(monkeypatch, engine=None):
    import torch
    real = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **kw: real(*a, **kw))
    eng = RecordingEngine() if engine is None else engine
    return eng, _bare(eng)


def _tet(**kw):
    c = _inputs()[0]
    return dict(_kinds()[0], basis=c.basis, num_components=4, reduction=c.reduction, **kw)


def _edge(m=3):
    a = mc.combined_case()                      # (the 68 edges the stored basis was built on)
    return dict(a["specs"][0], basis=a["bases"][0], num_components=m)


def _names(eng):
    return [c[0] for c in eng.calls]


def _calls(eng):
    """The recorded calls with the device pointers that the recorder does not know of masked as it masks the others."""
    where = {"hyper_iterate": (3,), "pdsolve_positions": (0,), "pdsolve_carry": (0,)}
    return [[c[0], [("pointer" if a is not None else None) if i in where.get(c[0], ()) else a for i, a in enumerate(c[1])]] + c[2:] for c in eng.calls]


def test_set_reduced_kinds_checks_its_limit(monkeypatch):
    eng, snaps = _patched(monkeypatch)
    for bad in (0, 9, -1, 2.0, 1.5, True, False, None, "2", [2]):
        with pytest.raises(ValueError, match="set_reduced_kinds"):
            snaps.set_reduced_kinds(bad)
    for good in (1, 8, np.int64(3)):
        snaps.set_reduced_kinds(good)
    snaps.set_reduced_kinds()
    assert snaps._reduced_limit == 1 and eng.calls == []


def test_refusals_fire_before_the_engine_is_touched(monkeypatch):
    eng, snaps = _patched(monkeypatch)
    m = snaps.mass
    two = [_tet(), _edge()]
    # the default limit, and limit 1 set explicitly: the parent's refusals, word for word
    for _ in range(2):
        with pytest.raises(ValueError, match="second reduced kind .*the engine holds one reduced operator"):
            snaps.solve_frames(two, 0.5, masses=m)
        with pytest.raises(ValueError, match="second reduced kind"):
            snaps.simulate_frames(two, 0.5, 2, masses=m)
        with pytest.raises(ValueError, match="every kind reduced.*exactly one kind"):
            snaps.solve_frames(two, 0.5, masses=m, hyper="touched")
        snaps.set_reduced_kinds(1)
    snaps.set_reduced_kinds(2)
    third = dict(_tet(), kind="tets_deformation_gradient")
    for call in (lambda **kw: snaps.solve_frames(two + [third], 0.5, masses=m, **kw), lambda **kw: snaps.simulate_frames(two + [third], 0.5, 2, masses=m, **kw)):
        with pytest.raises(ValueError, match="more than 2 reduced kinds.*set_reduced_kinds"):
            call()
        with pytest.raises(ValueError, match="more than 2 reduced kinds.*set_reduced_kinds"):
            call(hyper="all")
    for hyper in ("touched", "all"):
        with pytest.raises(ValueError, match="every kind reduced"):                 # a mixed list
            snaps.solve_frames([_tet(), _kinds()[1]], 0.5, masses=m, hyper=hyper)
        with pytest.raises(ValueError, match="every kind reduced"):
            snaps.simulate_frames([_kinds()[0], _edge()], 0.5, 2, masses=m, hyper=hyper)
        with pytest.raises(ValueError, match="history"):
            snaps.solve_frames(two, 0.5, masses=m, history=True, hyper=hyper)
    with pytest.raises(ValueError, match="hyper must be"):
        snaps.solve_frames(two, 0.5, masses=m, hyper="rows")
    with pytest.raises(ValueError, match="num_components"):
        snaps.solve_frames([_tet(), {k: v for k, v in _edge().items() if k != "num_components"}], 0.5, masses=m)
    with pytest.raises(ValueError, match="listed twice"):
        snaps.solve_frames([_tet(), _tet()], 0.5, masses=m)
    assert eng.calls == []


def test_one_reduced_kind_records_the_parents_sequence_whatever_the_limit(monkeypatch):
    calls = {
        "solve": lambda s, **kw: s.solve_frames([_tet(), _kinds()[1]], 0.5, num_iterations=3, frame_start=1, frame_jump=2, **kw),
        "solve_hyper": lambda s, **kw: s.solve_frames([_tet()], 0.5, num_iterations=3, chunk_frames=16, hyper="touched", **kw),
        "simulate": lambda s, **kw: s.simulate_frames([_kinds()[1], _tet()], 0.5, 3, num_iterations=2, record_every=2, **kw),
        "simulate_hyper": lambda s, **kw: s.simulate_frames([_tet()], 0.5, 2, num_iterations=2, hyper="all", **kw),
    }
    for name, call in calls.items():
        eng0, fresh = _patched(monkeypatch)
        call(fresh)
        eng1, snaps = _patched(monkeypatch)
        snaps.set_reduced_kinds(4)
        call(snaps)
        assert _calls(eng1) == _calls(eng0), name
        assert "rforce_bank" not in _names(eng1) and "rforce_operator" in _names(eng1)


def test_engine_calls_of_two_reduced_kinds(monkeypatch):
    head = ["gstep_held", "gstep_setup"]
    slots = ["rforce_bank", "cproj_setup", "rforce_solver", "pdsolve_slot"] * 2
    banks = lambda eng: [c[1][0] for c in eng.calls if c[0] == "rforce_bank"]
    two = [_tet(), _edge()]
    # solve_frames without hyper: S^T V per bank, the slots on their banks, the plain iteration, bank 0 again
    eng, snaps = _patched(monkeypatch)
    snaps.set_reduced_kinds(2)
    out, nF = snaps.solve_frames(two, 0.5, num_iterations=3, frame_start=1, frame_jump=2)
    assert _names(eng) == head + ["rforce_bank", "rforce_operator"] * 2 + ["pdsolve_begin"] + slots + ["pdsolve_iterate", "rforce_bank"]
    assert banks(eng) == [0, 1, 0, 1, 0] and tuple(out.shape) == (nF, snaps.nVerts, 3)
    assert list(snaps.assembly_ST) == ["tets_strain", "edge_spring"]
    # a third, plain kind in the middle keeps its list position and takes no bank
    eng, snaps = _patched(monkeypatch)
    snaps.set_reduced_kinds(8)
    snaps.solve_frames([_tet(), dict(_kinds()[0], kind="tets_deformation_gradient"), _edge()], 0.5, num_iterations=1)
    assert _names(eng) == head + ["rforce_bank", "rforce_operator"] * 2 + ["pdsolve_begin"] + slots[:4] + ["cproj_setup", "pdsolve_slot"] + slots[4:] \
        + ["pdsolve_iterate", "rforce_bank"]
    assert banks(eng) == [0, 1, 0, 1, 0]
    # with hyper: A^-1 S^T V per bank behind S^T V, ONE hyper_iterate on the union
    for hyper in ("touched", "all"):
        eng, snaps = _patched(monkeypatch)
        snaps.set_reduced_kinds(2)
        snaps.solve_frames(two, 0.5, num_iterations=3, chunk_frames=16, hyper=hyper)
        assert _names(eng) == head + ["rforce_bank", "rforce_operator", "hyper_operator"] * 2 + ["pdsolve_begin"] + slots + ["hyper_iterate", "rforce_bank"]
        assert banks(eng) == [0, 1, 0, 1, 0]
        n_iter, touched, chunk = eng.calls[-2][1][:3]
        assert n_iter == 3 and chunk == 16 and (touched is None) == (hyper == "all")
        if hyper == "touched":          # ONE list, the union of the two kinds' touched vertices
            a = mc.combined_case()
            union, _, own = mc.sampled(a, {0: a["op"](0, 3), 1: a["op"](1, 4)})
            assert touched[0] == [union.shape[0]] and max(v.shape[0] for v in own.values()) < union.shape[0] < snaps.nVerts
    # simulate_frames: the operators once, the slots once, per step one iterate; state= and record_every as ever
    for hyper in (None, "touched"):
        eng, snaps = _patched(monkeypatch)
        snaps.set_reduced_kinds(2)
        q, q_prev, nF, (records, steps) = snaps.simulate_frames(two, 0.5, 3, num_iterations=2, record_every=2, chunk_frames=16, hyper=hyper)
        ops = ["rforce_bank", "rforce_operator"] + (["hyper_operator"] if hyper else [])
        it = "hyper_iterate" if hyper else "pdsolve_iterate"
        assert _names(eng) == head + ops * 2 + ["pdsolve_begin", "pdsolve_carry"] + slots + [it, "pdsolve_advance", it, "pdsolve_advance", it] \
            + ["pdsolve_positions", "rforce_bank"]
        assert banks(eng) == [0, 1, 0, 1, 0] and steps == [2] and tuple(records.shape) == (1, nF, snaps.nVerts, 3)


class _Raising(RecordingEngine):
    """Raises in the named call, after recording it."""
    def __init__(self, where):
        RecordingEngine.__init__(self)
        self._where = where

    def __getattr__(self, name):
        call = RecordingEngine.__getattr__(self, name)
        if name != self._where:
            return call

        def boom(*a, **kw):
            call(*a, **kw)
            raise RuntimeError("engine failure in " + name)
        return boom


@pytest.mark.parametrize("where", ["rforce_operator", "hyper_operator", "pdsolve_begin", "pdsolve_slot", "hyper_iterate", "pdsolve_iterate"])
def test_a_raising_engine_leaves_bank_zero_current(monkeypatch, where):
    hyper = None if where == "pdsolve_iterate" else "touched"
    for call in (lambda s: s.solve_frames([_tet(), _edge()], 0.5, num_iterations=2, hyper=hyper),
                 lambda s: s.simulate_frames([_tet(), _edge()], 0.5, 2, num_iterations=2, hyper=hyper)):
        eng, snaps = _patched(monkeypatch, _Raising(where))
        snaps.set_reduced_kinds(2)
        with pytest.raises(RuntimeError, match="engine failure"):
            call(snaps)
        assert eng.calls[-1][0] == "rforce_bank" and eng.calls[-1][1] == [0]
        # ... and the next single-kind call on this object behaves as on a fresh one
        eng.calls, eng._where = [], None
        snaps.solve_frames([_tet()], 0.5, num_iterations=2, hyper="touched")
        eng0, fresh = _patched(monkeypatch)
        fresh.solve_frames([_tet()], 0.5, num_iterations=2, hyper="touched")
        assert _calls(eng) == _calls(eng0)


def test_the_docstrings_name_the_setter():
    from animsnapbases_amd.posSnapshots import posSnapshots
    flat = lambda fn: " ".join(fn.__doc__.split())
    for fn in (posSnapshots.solve_frames, posSnapshots.simulate_frames):
        assert "``set_reduced_kinds(L)``" in flat(fn)
    assert "every kind must be reduced, which without ``set_reduced_kinds`` means exactly one kind" in flat(posSnapshots.solve_frames)
    setter = flat(posSnapshots.set_reduced_kinds)
    for words in ("an integer 1..8", "1, the default: one reduced kind", "the i-th on the engine's bank i", "EVERY listed kind reduced",
                  "keep their one kind", "Checked before the device is touched"):
        assert words in setter, words
    for fn in (posSnapshots.reduced_force_errors, posSnapshots.reduced_global_step_errors, posSnapshots.reduced_solve_errors,
               posSnapshots.reduced_rollout_errors):
        assert "one kind whatever ``set_reduced_kinds`` allows: multi-kind sweeps are out of scope" in flat(fn), fn.__name__


# ------------------------------------------------------------------ 5. the ABI
def test_new_abi_names_are_declared():
    import os
    import re
    from conftest import ROOT
    assert "asb_rforce_bank" in _lib.PROTOTYPES and hasattr(_lib.load(), "asb_rforce_bank")
    text = open(os.path.join(ROOT, "include", "asb.h")).read()
    assert re.search(r"#define\s+ASB_RFORCE_BANKS\s+8\b", text)
    assert re.search(r"\bint\s+asb_rforce_bank\s*\(\s*asb_ctx\s*\*\s*ctx\s*,\s*int\s+bank\s*\)\s*;", text)
    from animsnapbases_amd.engine import HipEngine
    assert callable(getattr(HipEngine, "rforce_bank"))
