"""CPU: the engine calls of the resident-dynamics methods of ``posSnapshots`` (constraint projections and forces, their DEIM
reduction, the solver iterations), pinned call by call.  A bare ``posSnapshots`` drives a recording double of the engine:
every engine method called is recorded with its name and arguments -- scalars as they are, arrays as (shape, dtype, sha1 of
the bytes), CSR matrices as the three arrays, a ``ProjectionSetup`` as its four arrays, device pointers as "pointer" -- so the
sequence is what the device is handed and in which order.  ``tests/dynamics_trace.json`` holds the sequences as recorded at
commit 81c7ae9, before these methods moved into ``animsnapbases_amd/dynamics.py``; a digest that differs means the device is
handed something else.  ``python tests/test_dynamics_trace_cpu.py --record`` rewrites the file (only when a change of the
trace is the purpose).

Inputs: the 18-vertex fixture ``cproj_tets_strain`` (tets_strain), edge springs on the edges of its tetrahedra, the basis of
``reduced_forces_tets_deim``; mass weighting and standardisation are on, so invMassL, add_mean and psf are not trivial.
``global_step``, ``global_solve`` and ``reduced_global_step_errors`` insist on a device tensor and stay with the GPU tests."""
import hashlib
import json
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
TRACES = os.path.join(HERE, "dynamics_trace.json")
# engine method -> the positions of its device-pointer arguments
POINTERS = {"cproj_run": (9,), "cforce_run": (12,), "rforce_run": (10,), "gstep_inertia": (10,), "pdsolve_begin": (11,),
            "pdsolve_iterate": (2,), "force_diff": (0, 1), "gstep_run": (0, 2)}


def _digest(x):
    from scipy import sparse
    from animsnapbases_amd.projections import ProjectionSetup
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    if isinstance(x, np.generic):
        return x.item()
    if isinstance(x, ProjectionSetup):
        return {"setup": [_digest(a) for a in (x.idx, x.table, x.star_ptr, x.star_idx)]}
    if sparse.issparse(x):
        return {"csr": [list(x.shape)] + [_digest(a) for a in (x.indptr, x.indices, x.data)]}
    if isinstance(x, (list, tuple)):
        return [_digest(a) for a in x]
    a = np.ascontiguousarray(x)
    return [list(a.shape), str(a.dtype), hashlib.sha1(a.tobytes()).hexdigest()]


class RecordingEngine(object):
    """Records (name, arguments) of every engine method called; answers what the callers read back."""
    device_id = 0

    def __init__(self):
        self.calls = []
        self._frames = None

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*args, **kw):
            rec = [("pointer" if a is not None else None) if i in POINTERS.get(name, ()) else _digest(a) for i, a in enumerate(args)]
            self.calls.append([name, rec] + ([{k: _digest(kw[k]) for k in sorted(kw)}] if kw else []))
            return getattr(self, "_" + name, lambda *a, **k: None)(*args, **kw)
        return call

    def _gstep_setup(self, A):
        return 0.0

    def _pdsolve_begin(self, which, f0, f1, fj, *rest):
        self._frames = len(range(f0, f1, fj))

    def _pdsolve_iterate(self, n_iter, chunk_frames=0, out_dev_ptr=None, history=False):
        return np.ones((n_iter, self._frames, 2))

    def _force_diff(self, a, b, F, N, per_frame=False):
        return np.ones(3), 1.0, np.ones(4), np.ones((F, 2)) if per_frame else None


def _inputs():
    from conftest import load_golden
    from reduced_forces_cases import case
    c = case("tets_deim")
    g = load_golden("cproj_tets_strain")
    tets = g["elements"]
    edges = np.unique(np.sort(np.concatenate([tets[:, [i, j]] for i in range(4) for j in range(i + 1, 4)]), axis=1), axis=0)
    return c, g, tets, edges


def _bare(eng):
    from animsnapbases_amd.posSnapshots import posSnapshots
    _, g, _, _ = _inputs()
    frames = np.array(g["frames"])
    F, N = frames.shape[:2]
    snaps = posSnapshots.__new__(posSnapshots)
    snaps._engine, snaps._comm = eng, types.SimpleNamespace(multi=False)
    snaps.frs, snaps.nVerts = F, N
    snaps.verts, snaps.tris, snaps.test_verts, snaps._snapTensor = frames, None, None, None
    snaps.mass = 0.5 + np.random.default_rng(5).random(N)
    snaps.massL = np.sqrt(snaps.mass)
    snaps.invMassL = 1.0 / snaps.massL
    snaps._standarize, snaps.pre_scale_factor = True, 2.5
    snaps.mean = frames[0] * snaps.massL[:, None]
    snaps.assembly_ST = snaps.bending_indices = snaps.global_matrix = snaps.global_solve_residual = None
    return snaps


def _kinds():
    c, g, tets, edges = _inputs()
    smin, smax = (float(s) for s in g["sigma"])
    tet = dict(kind="tets_strain", elements=tets, wi=0.7, rest_positions=g["rest"], sigma_min=smin, sigma_max=smax)
    return tet, dict(kind="edge_spring", elements=edges, wi=1.3)          # (the springs rest at frame 0 of the animation)


def _reduced_kw(**kw):
    c, _, _, _ = _inputs()
    tet = {k: v for k, v in _kinds()[0].items() if k != "kind"}
    return dict(tet, reduction=c.reduction, **kw)


def _held_out():
    return np.ascontiguousarray(_inputs()[1]["frames"][::-1]) * 1.01


# name -> the public call on a bare posSnapshots
CALLS = {
    "constraint_projections": lambda s: s.constraint_projections("tets_strain", **{k: v for k, v in _kinds()[0].items() if k != "kind"}),
    "constraint_forces_train": lambda s: s.constraint_forces(list(_kinds()), frame_start=1, frame_jump=2, chunk_frames=16),
    "constraint_forces_array": lambda s: s.constraint_forces(list(_kinds()), animation=_held_out(), frame_start=1, frame_jump=2,
                                                             chunk_frames=16),
    "reduced_constraint_forces": lambda s: s.reduced_constraint_forces("tets_strain", _inputs()[0].basis, 4, **_reduced_kw()),
    "reduced_force_errors": lambda s: s.reduced_force_errors("tets_strain", _inputs()[0].basis, [2, 4, 3], **_reduced_kw(per_frame=True)),
    "reduced_force_errors_empty": lambda s: s.reduced_force_errors("tets_strain", _inputs()[0].basis, [], **_reduced_kw()),
    "solve_frames": lambda s: s.solve_frames([dict(_kinds()[0], basis=_inputs()[0].basis, num_components=4, reduction=_inputs()[0].reduction),
                                              _kinds()[1]], 0.5, num_iterations=3, gravity=(0.0, -9.81, 0.0), start="frame",
                                             frame_start=1, frame_jump=2, history=True),
    "reduced_solve_errors": lambda s: s.reduced_solve_errors("tets_strain", _inputs()[0].basis, [2, 4], 0.5, num_iterations=2,
                                                             velocity="zero", animation=_held_out(), **_reduced_kw()),
}


def _result(x):
    """What a call returns, device tensors as their shapes."""
    import torch
    if isinstance(x, torch.Tensor):
        return {"tensor": list(x.shape), "dtype": str(x.dtype)}
    if isinstance(x, (list, tuple)) and not (x and all(isinstance(v, float) for v in x)):
        return [_result(v) for v in x]
    return _digest(x)


def _trace(name, monkeypatch, counts=None):
    """The engine calls of ``CALLS[name]`` on a fresh bare object, what it returned and the attributes it left."""
    import torch
    from animsnapbases_amd import projections
    real = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **kw: real(*a, **kw))
    if counts is not None:
        for fn in ("build_setup", "assembly_ST"):
            def counted(*a, _fn=fn, _real=getattr(projections, fn), **kw):
                counts[_fn] = counts.get(_fn, 0) + 1
                return _real(*a, **kw)
            monkeypatch.setattr(projections, fn, counted)
    eng = RecordingEngine()
    snaps = _bare(eng)
    out = CALLS[name](snaps)
    left = {"assembly_ST": None if snaps.assembly_ST is None else {k: _digest(v) for k, v in sorted(snaps.assembly_ST.items())},
            "bending_indices": _digest(snaps.bending_indices), "global_matrix": _digest(snaps.global_matrix),
            "global_solve_residual": snaps.global_solve_residual}
    return json.loads(json.dumps({"calls": eng.calls, "returned": _result(out), "left": left}))


@pytest.mark.parametrize("name", sorted(CALLS))
def test_engine_calls_are_the_recorded_ones(name, monkeypatch):
    with open(TRACES) as fh:
        want = json.load(fh)
    assert want["recorded_at_commit"] == "81c7ae9"
    got = _trace(name, monkeypatch)
    assert [c[0] for c in got["calls"]] == [c[0] for c in want["traces"][name]["calls"]]
    for i, (a, b) in enumerate(zip(got["calls"], want["traces"][name]["calls"])):
        assert a == b, "call %d (%s)" % (i, a[0])
    assert got == want["traces"][name]


def test_the_traces_cover_what_they_are_meant_to():
    """The recorded sequences themselves: the kinds in list order, one reduced run per r, nothing on an empty ``r_values``."""
    with open(TRACES) as fh:
        t = json.load(fh)["traces"]
    names = lambda k: [c[0] for c in t[k]["calls"]]
    assert names("constraint_projections") == ["cproj_setup", "cproj_run"]
    assert names("constraint_forces_train") == 2 * ["cproj_setup", "cforce_run"]
    assert names("constraint_forces_array") == ["heldout_upload"] + 2 * ["cproj_setup", "cforce_run"]
    assert names("reduced_constraint_forces") == ["rforce_operator", "cproj_setup", "rforce_solver", "rforce_run"]
    assert names("reduced_force_errors") == ["cproj_setup", "cforce_run", "rforce_operator"] \
        + 3 * ["cproj_setup", "rforce_solver", "rforce_run", "force_diff"]
    assert names("reduced_force_errors_empty") == []
    assert names("solve_frames") == ["gstep_held", "gstep_setup", "rforce_operator", "pdsolve_begin", "cproj_setup", "rforce_solver",
                                     "pdsolve_slot", "cproj_setup", "pdsolve_slot", "pdsolve_iterate"]
    full = ["heldout_upload", "pdsolve_begin", "cproj_setup", "pdsolve_slot", "pdsolve_iterate"]
    reduced = ["heldout_upload", "pdsolve_begin", "cproj_setup", "rforce_solver", "pdsolve_slot", "pdsolve_iterate", "force_diff"]
    assert names("reduced_solve_errors") == ["gstep_held", "gstep_setup"] + full + ["rforce_operator"] + 2 * reduced


@pytest.mark.parametrize("name,kinds", [("reduced_force_errors", 1), ("solve_frames", 2), ("reduced_solve_errors", 1)])
def test_each_kind_is_set_up_once_per_public_call(name, kinds, monkeypatch):
    """``projections.build_setup`` and ``assembly_ST`` run once per kind per public call: the reduced operator takes the term the
    plan already made."""
    counts = {}
    _trace(name, monkeypatch, counts)
    assert counts == {"build_setup": kinds, "assembly_ST": kinds}


def _dump(doc, fh):
    """One engine call per line."""
    js = lambda x: json.dumps(x, sort_keys=True)
    fh.write('{"recorded_at_commit": %s, "traces": {\n' % js(doc["recorded_at_commit"]))
    for i, (name, t) in enumerate(sorted(doc["traces"].items())):
        fh.write(' %s: {"calls": [\n%s],\n  "left": %s,\n  "returned": %s}%s\n'
                 % (js(name), ",\n".join("   " + js(c) for c in t["calls"]), js(t["left"]), js(t["returned"]),
                    "," if i + 1 < len(doc["traces"]) else ""))
    fh.write("}}\n")


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    sys.path.insert(0, os.path.dirname(HERE))
    mp = pytest.MonkeyPatch()
    traces = {}
    for n in sorted(CALLS):
        traces[n] = _trace(n, mp)
        mp.undo()
    with open(TRACES, "w") as fh:
        _dump({"recorded_at_commit": "81c7ae9", "traces": traces}, fh)
