"""CPU: the fixtures of tools/gen_golden_pdsolve.py -- q after K in {1, 3, 10} iterations of the UNMODIFIED reference's loop
(Simulators.py:506-526) -- against the NumPy model of tests/pdsolve_cases.py within B_K = 2 K max(1, amp) (one-iteration
bound), which shows fixtures and bounds sound without a device; the argument checks of ``posSnapshots.solve_frames`` and
``reduced_solve_errors``, which fire before the engine is touched; the several-ranks refusal; the new names of the C ABI."""
import types

import numpy as np
import pytest

from conftest import load_golden
from pdsolve_cases import AMP_CAP, KS, MODES, NAMES, bound_K, host_case, model
from test_gpu_gstep import _case as gstep_case

from animsnapbases_amd import _lib
from animsnapbases_amd.posSnapshots import posSnapshots


@pytest.mark.parametrize("name", NAMES)
def test_host_model_matches_the_reference_loop(name):
    z = load_golden("pdsolve_" + name)
    assert z["Ks"].tolist() == list(KS) and float(z["dt"]) == 0.5 and float(z["wi"]) == 0.7
    _, frames, _, one = gstep_case(name)
    c = host_case(name)
    assert np.array_equal(c["frames"], frames)
    F = frames.shape[0]
    for mode in MODES:
        got = model(c, range(F), mode, KS)
        for K in KS:
            amp = float(z["amp_%s_%d" % (mode, K)])
            assert 0.0 < amp <= AMP_CAP
            ref = z["q_%s_%d" % (mode, K)]
            assert ref.shape == frames.shape and np.isfinite(ref).all()
            B = bound_K(one[mode], K, amp)
            err = np.abs(got[K] - ref).max()                        # over every frame: none is left out
            print("%s %s K = %d: amp %.3g, max abs err %.3g, B_K %.3g, err / bound %.3g" % (name, mode, K, amp, err, B, err / B))
            assert err <= B
        # the iterations move: the fixture tells K = 1 from K = 10
        assert np.abs(z["q_%s_10" % mode] - z["q_%s_1" % mode]).max() > bound_K(one[mode], 10, float(z["amp_%s_10" % mode]))


def test_one_model_iteration_from_the_frame_is_the_recorded_global_step():
    z, frames, _, one = gstep_case("tets_strain")
    c = host_case("tets_strain")
    for mode in MODES:
        got = model(c, range(frames.shape[0]), mode, (1,), start="frame")[1]
        assert np.abs(got - z["q_" + mode]).max() <= one[mode]


def _bare(multi):
    snaps = posSnapshots.__new__(posSnapshots)
    snaps._comm = types.SimpleNamespace(multi=multi)
    return snaps


def test_several_ranks_are_refused():
    g = load_golden("cproj_tets_strain")
    kinds = [dict(kind="tets_strain", elements=g["elements"])]
    snaps = _bare(True)
    with pytest.raises(NotImplementedError):
        snaps.solve_frames(kinds, 0.5, masses=np.ones(g["rest"].shape[0]))
    with pytest.raises(NotImplementedError):
        snaps.reduced_solve_errors("tets_strain", {}, [1], 0.5, masses=np.ones(g["rest"].shape[0]))


def test_arguments_checked_before_the_device_is_touched():
    snaps = _bare(False)                                            # no engine: touching it is an AttributeError
    snaps.mass, snaps.global_matrix = None, None
    m = np.ones(4)
    edge = dict(kind="edge_spring", elements=np.array([[0, 1]]))
    for call in (lambda **kw: snaps.solve_frames([edge], kw.pop("dt", 0.5), **kw),
                 lambda **kw: snaps.reduced_solve_errors("edge_spring", {}, [1], kw.pop("dt", 0.5), **kw)):
        with pytest.raises(ValueError, match="masses"):
            call()
        with pytest.raises(ValueError, match="velocity"):
            call(masses=m, velocity="leapfrog")
        with pytest.raises(ValueError, match="gravity"):
            call(masses=m, gravity=(0.0, np.nan, 0.0))
        with pytest.raises(ValueError, match="dt"):
            call(masses=m, dt=0.0)
        for K in (0, -1, 2.5, None, "ten"):
            with pytest.raises(ValueError, match="num_iterations"):
                call(masses=m, num_iterations=K)
        for start in ("rest", None, np.zeros((1, 4, 3)), 3):
            with pytest.raises(ValueError, match="start"):
                call(masses=m, start=start)
    import torch
    for bad in (torch.zeros((1, 4, 3), dtype=torch.float64), torch.zeros((1, 4, 3), dtype=torch.float32)):      # host tensors
        with pytest.raises(ValueError, match="start"):
            snaps.solve_frames([edge], 0.5, masses=m, start=bad)
    # the kinds: unknown keys, the reduction keys incomplete, a second reduced kind
    snaps.nVerts, snaps.frs, snaps.verts, snaps.tris = 4, 3, np.zeros((3, 4, 3)), None
    with pytest.raises(ValueError, match="unknown key"):
        snaps.solve_frames([dict(edge, stiffness=2.0)], 0.5, masses=m)
    with pytest.raises(ValueError, match="num_components"):
        snaps.solve_frames([dict(edge, basis={})], 0.5, masses=m)
    with pytest.raises(ValueError, match="second reduced kind"):
        snaps.solve_frames([dict(edge, basis={}, num_components=1), dict(kind="tris_strain", elements=np.array([[0, 1, 2]]), basis={},
                                                                         num_components=1)], 0.5, masses=m)
    with pytest.raises(ValueError, match="non-empty list"):
        snaps.solve_frames([], 0.5, masses=m)
    with pytest.raises(ValueError, match="non-empty list"):
        snaps.solve_frames(None, 0.5, masses=m)


def test_new_abi_names_are_declared():
    for name in ("asb_pdsolve_begin", "asb_pdsolve_slot", "asb_pdsolve_iterate"):
        assert name in _lib.PROTOTYPES
        assert hasattr(_lib.load(), name)
