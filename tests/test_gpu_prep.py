"""GPU (-m gpu): the snapshot preparation -- csrc/asb_snapshots.hip and posSnapshots.standarize -- against the models of
prep_model.py on the case table of prep_cases.py, read back through asb_test_prep_state.

 1. layout and rest shape: the four ingest calls on every row of the table; the raw vertex-major tensor WITH its padding and
    the rest shape equal the order model to the last bit (so the padding is == 0 and the four calls agree bit for bit); the
    download equals the raw rows; the padding stays zero when the context held a longer tensor of 1e30 before a fused call.
 2. sums: sum(x), sum(x^2) (fused, rest shape 0), sum (x - mu)^2 for mu = 0, the mean and 1e3 x the spread: == on the integer
    rows, within the bound of prep_model on the float rows; the n_loc = 11 000 rows run the capped grids, which is asserted from
    nblk_cap as read from asb_test_deflate_state.
 3. scaling sweep: tensor to the bit; E0, EV, |X|^2, max E0, mean_energy, mean_frac, sum EV, sum EV^2, ev_cv2 against the model;
    the flags; a second scale; every later writer of X clears the flags; asb_panel_guess_stats; the projection mode's initial
    energies are E0 bit for bit, and with ASB_E0_REUSE=0 (read per context: no child process) within the bound of E0.
 4. standarize() end to end on generic, offset and translated data, both rest shapes, with and without mass: pre_scale_factor
    within its bound of longdouble 1 / std, the branch as predicted (a counter around the engine's sqdev), the prepared tensor
    == the order model times the device's own factor; the same on two thread ranks with an uneven split.
 5. held-out preparation of the training frames against the training tensor within 2 eps (|m x| + |mean|) |a|; how many
    entries differ in their last bit is printed (k_heldout_prep may contract x m - mean into one FMA), not asserted.
 6. n_loc = 700 000, F = 1: upload, download and residual download with == (more than 65 535 strips of 32 rows).

Every bound comes from prep_model.py (derivations in its docstring); none is a number taken from the device.  Each test prints
achieved / bound; OBSERVED holds the largest ratio per group as measured on the MI355X (test_zz_observed prints this run's).
"""
import contextlib
import io

import numpy as np
import pytest

import prep_cases as pc
import prep_model as pm
from animsnapbases_amd import _lib

pytestmark = pytest.mark.gpu

U = pm.U
PATHS = ("host", "host_fused", "device", "device_fused")

# largest achieved / bound per group, measured on the MI355X (0 where every comparison was exact).  A record for the reader, copied
# by hand from the printout of test_zz_observed: no code reads it and no bound is taken from it.
OBSERVED = {
    "sum(x)": 0.022, "sum(x^2) fused": 0.034, "sum (x - mu)^2": 0.077,
    "E0 per vertex": 0.102, "EV per vertex": 0.086, "|X|^2 = sum E0": 0.102, "|X|^2 vs model": 0.069,
    "mean_energy = sum m_v": 0.041, "sum EV": 0.077, "sum EV^2": 0.068, "sum EV vs model": 0.063, "sum EV^2 vs model": 0.067,
    "mean_frac": 0.046, "ev_cv2": 0.030,
    "pre_scale_factor one sweep": 0.029, "pre_scale_factor second pass": 0.116, "pre_scale_factor two ranks": 0.044,
    "held-out vs training": 0.0, "recomputed energy vs model": 0.031,
}

_SEEN = {}
_CAP = []


def _note(group, achieved, bound):
    achieved, bound = float(achieved), float(bound)
    ratio = 0.0 if achieved == 0.0 else (achieved / bound if bound > 0 else np.inf)
    _SEEN[group] = max(_SEEN.get(group, 0.0), ratio)
    print("  %-28s achieved %.3e  bound %.3e  ratio %.3f" % (group, achieved, bound, ratio))
    return achieved <= bound


def _engine():
    from animsnapbases_amd import HipEngine
    return HipEngine(0)


def _cap():
    if not _CAP:
        e = _engine()
        e.upload(np.ones((1, 1, 3)), 0, 1)
        e.deflate_begin(1, False)
        _CAP.append(e.test_deflate_state()["nblk_cap"])
        e.close()
        assert _CAP[0] >= 8
    return _CAP[0]


def _ingest(e, path, X, massL, r, keep):
    """one ingest call on engine e -> (sum, sum of squares or None)"""
    import torch
    if path.startswith("device"):
        shard = torch.from_numpy(np.ascontiguousarray(X[:, r.v0:r.v0 + r.n_loc])).to("cuda:0")
        torch.cuda.synchronize()
        keep.append(shard)
        m_loc = None if massL is None else massL[r.v0:r.v0 + r.n_loc]
    if path == "host":
        e.upload(X, r.v0, r.n_loc, massL)
        return e.center(r.code, r.subtract), None
    if path == "host_fused":
        return e.upload_rest(X, r.v0, r.n_loc, massL, r.code, r.subtract)
    if path == "device":
        e.adopt_device(shard.data_ptr(), r.F, r.n_loc, m_loc, r.v0, r.N)
        return e.center(r.code, r.subtract), None
    return e.adopt_device_rest(shard.data_ptr(), r.F, r.n_loc, m_loc, r.v0, r.N, r.code, r.subtract)


def _check_large(r):
    if r.n_loc == pc.N_LARGE:
        facts = pc.large_grid_facts(_cap())
        assert all(facts.values()), facts


# ------------------------------------------------------------------------------------------------ 1, 2
@pytest.mark.parametrize("r", pc.ROWS, ids=pc.row_id)
def test_layout_rest_shape_and_sums(r):
    _check_large(r)
    cap = _cap()
    X, massL = pc.data(r)
    want, want_mean = pm.order_tensor(X, massL, r.v0, r.n_loc, r.code, r.subtract)
    raw = pm.vertex_major(want)
    exact = r.family == "integer"
    if exact:
        assert pm.fits53(want)
    ref = pm.ld_sums(want)
    e, keep = _engine(), []
    try:
        for p in PATHS:
            s, s2 = _ingest(e, p, X, massL, r, keep)
            st = e.test_prep_state(want_X=True, want_energies=False)
            assert (st["X"][:, :, r.F:] == 0).all(), "%s: the padding is not zero" % p
            assert pm.same_bits(st["X"], raw), "%s: the raw tensor differs from the order model" % p
            assert pm.same_bits(e.get_mean(), want_mean), "%s: the rest shape differs from the order model" % p
            assert st["have_mean"] and not st["e0_valid"] and not st["ev_valid"]
            assert pm.same_bits(e.download_snapshots(), st["X"][:, :, :r.F].transpose(2, 0, 1)), "%s: download != raw rows" % p
            fused0 = p.endswith("fused") and r.code == 0
            assert (s2 is not None) == fused0
            depth = pm.depth_fused(r.F, r.n_loc) if fused0 else pm.depth_rows(r.F, r.n_loc, cap)
            if exact:
                assert s == float(ref["sum"]) and (s2 is None or s2 == float(ref["sq"])), (p, s, s2)
            else:
                assert _note("sum(x)", abs(s - ref["sum"]), pm.sum_bound(depth, ref["abs"])), p
                if s2 is not None:
                    assert _note("sum(x^2) fused", abs(s2 - ref["sq"]), pm.sum_bound(depth, ref["sq"], extra=1)), p
        # sum (x - mu)^2 on the tensor the last call left
        mu_true, var, std = pm.ld_std(want)
        mus = (0.0, 3.0) if exact else (0.0, float(mu_true), float(mu_true + 1e3 * std))
        for mu in mus:
            got = e.sqdev(mu)
            sd = pm.ld_sums(want, mu)["sqdev"]
            if exact:
                assert got == float(sd), (mu, got, float(sd))
            else:
                assert _note("sum (x - mu)^2", abs(got - sd), pm.sum_bound(pm.depth_rows(r.F, r.n_loc, cap), sd, extra=3)), mu
    finally:
        e.close()


@pytest.mark.parametrize("F_before", (100, 31))
@pytest.mark.parametrize("path", ("host_fused", "device_fused"))
def test_padding_is_zero_after_a_longer_tensor_of_1e30(path, F_before):
    """the fused calls skip the clearing memset: k_transpose_first alone writes the padding.  F_before = 31: the same allocation
    is kept (Fp = 32 both times) and its columns 17 .. 30 held 1e30; F_before = 100: a shorter row length in the same context"""
    n = 43
    r = pc.Row(17, n, n, 0, True, 0, True, "integer")
    X, massL = pc.integer_data(r)
    e, keep = _engine(), []
    try:
        e.upload(np.full((F_before, n, 3), 1e30), 0, n)
        assert (e.test_prep_state(want_X=True, want_energies=False)["X"][:, :, :F_before] == 1e30).all()
        _ingest(e, path, X, massL, r, keep)
        st = e.test_prep_state(want_X=True, want_energies=False)
        assert (st["X"][:, :, 17:] == 0).all()
        want, _ = pm.order_tensor(X, massL, 0, n, 0, True)
        assert pm.same_bits(st["X"], pm.vertex_major(want))
        e.scale(2.0)                # ... and E0 over all Fp columns equals the model over the F columns
        E0, _, EV = pm.ev_integer_model(want * 2.0)
        st = e.test_prep_state()
        assert np.array_equal(st["E0"], E0) and np.array_equal(st["EV"], EV)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 3
def _check_energies(e, T, r, exact):
    """the state after a scaling sweep against the model of the scaled tensor T (F, n, 3)"""
    cap = _cap()
    n = r.n_loc
    st = e.test_prep_state(want_X=True)
    assert pm.same_bits(st["X"], pm.vertex_major(T)), "the scaled tensor differs from the order model"
    assert st["e0_valid"] and st["ev_valid"] and st["have_mean"]
    assert np.isfinite(st["E0"]).all() and np.isfinite(st["EV"]).all() and (st["EV"] >= 0).all()
    en = pm.ld_energies(T)
    bE0, bmv, bEV = pm.energy_bounds(en)
    sc = st["sc"]
    if exact:
        E0, mv, EV = pm.ev_integer_model(T)
        assert np.array_equal(st["E0"], E0) and np.array_equal(st["EV"], EV)
        assert sc[0] == E0.sum() and float(en["E0"].sum()) == E0.sum()
    else:
        assert (np.abs(st["E0"] - en["E0"]) <= bE0).all() and (np.abs(st["EV"] - en["EV"]) <= bEV).all()
        i, j = int(np.argmax(np.abs(st["E0"] - en["E0"]) - bE0)), int(np.argmax(np.abs(st["EV"] - en["EV"]) - bEV))
        _note("E0 per vertex", abs(st["E0"][i] - en["E0"][i]), bE0[i])
        _note("EV per vertex", abs(st["EV"][j] - en["EV"][j]), bEV[j])
    assert sc[1] == st["E0"].max(), "the largest energy is not the maximum of E0"
    # the reductions on the device's own arrays, then against the model
    dE0, dEV = st["E0"].astype(pm.LD), st["EV"].astype(pm.LD)
    dt, dm = pm.depth_totals(n, cap), pm.depth_moments(n)
    assert _note("|X|^2 = sum E0", abs(sc[0] - dE0.sum()), pm.sum_bound(dt, dE0.sum()))
    assert _note("sum EV", abs(sc[4] - dEV.sum()), pm.sum_bound(dm, dEV.sum()))
    assert _note("sum EV^2", abs(sc[5] - (dEV * dEV).sum()), pm.sum_bound(dm, (dEV * dEV).sum(), extra=1))
    b0 = pm.sum_bound(dt, en["E0"].sum()) + float(bE0.sum())
    b2 = pm.sum_bound(dt, en["mv"].sum()) + float(bmv.sum())
    b4 = pm.sum_bound(dm, en["EV"].sum()) + float(bEV.sum())
    b5 = pm.sum_bound(dm, (en["EV"] ** 2).sum(), extra=1) + float((2 * en["EV"] * bEV + bEV * bEV).sum())
    assert _note("|X|^2 vs model", abs(sc[0] - en["E0"].sum()), b0)
    assert _note("mean_energy = sum m_v", abs(sc[2] - en["mv"].sum()), b2)
    assert _note("sum EV vs model", abs(sc[4] - en["EV"].sum()), b4)
    assert _note("sum EV^2 vs model", abs(sc[5] - (en["EV"] ** 2).sum()), b5)
    assert st["prep_normx2"] == sc[0] and st["mean_energy"] == sc[2]
    if en["E0"].sum() > 0:
        frac = en["mv"].sum() / en["E0"].sum()
        assert _note("mean_frac", abs(st["mean_frac"] - frac), pm.quotient_bound(en["mv"].sum(), en["E0"].sum(), b2, b0))
    else:
        assert st["mean_frac"] == 0.0
    if sc[4] > 0 and n > 1:
        S1, S2 = en["EV"].sum(), (en["EV"] ** 2).sum()
        if S1 > 0:
            assert _note("ev_cv2", abs(st["ev_cv2"] - (pm.LD(n) * S2 / (S1 * S1) - 1)), pm.cv2_bound(n, S1, S2, b4, b5))
    else:
        assert st["ev_cv2"] == 0.0
    # no projection-mode run has begun on this context: a guessed first panel is not possible, the answer is (0, 0)
    # (the possible case: test_projection_mode_starts_from_E0_bit_for_bit)
    assert e.panel_guess_stats() == (0.0, 0.0, False)
    return st


@pytest.mark.parametrize("r", pc.ROWS, ids=pc.row_id)
def test_scaling_sweep(r):
    _check_large(r)
    X, massL = pc.data(r)
    want, _ = pm.order_tensor(X, massL, r.v0, r.n_loc, r.code, r.subtract)
    exact = r.family == "integer"
    e, keep = _engine(), []
    try:
        _ingest(e, "host_fused" if r.F % 2 else "device_fused", X, massL, r, keep)
        a = 4.0 if exact else 0.37
        e.scale(a)
        T = want * a
        _check_energies(e, T, r, exact)
        b = 0.5 if exact or r.F % 3 else 1.9       # a second scale multiplies again and refreshes the energies
        e.scale(b)
        _check_energies(e, T * b, r, exact)
    finally:
        e.close()


@pytest.mark.parametrize("kind", ("still", "still-raw", "one", "all", "offset-raw"))
def test_scaling_sweep_on_degenerate_energies(kind):
    """still vertices: E0 = EV = 0 exactly after the subtraction, E0 ~ m_v without it (EV >= 0, finite, within the bound of 0);
    one vertex carrying all the motion: ev_cv2 ~ n - 1; the same motion on every vertex: ev_cv2 ~ 0; offset data without the
    subtraction: E0 - m_v cancels"""
    F, n = 33, 50
    subtract = kind in ("still", "one", "all")
    if kind == "offset-raw":
        X = pc.offset_data(F, n)
    else:
        X = pc.still_data(F, n, moving={"one": (7,), "all": range(n)}.get(kind, ()))
    r = pc.Row(F, n, n, 0, False, 1 if kind != "still" else 0, subtract, "generic")
    want, _ = pm.order_tensor(X, None, 0, n, r.code, subtract)
    e = _engine()
    try:
        e.upload_rest(X, 0, n, None, r.code, subtract)
        e.scale(0.37)
        st = _check_energies(e, want * 0.37, r, False)
        if kind == "still":
            assert (st["E0"] == 0).all() and (st["EV"] == 0).all() and st["ev_cv2"] == 0.0 and st["mean_frac"] == 0.0
        if kind == "one":
            assert abs(st["ev_cv2"] - (n - 1)) < 1e-6 * n
        if kind == "all":
            assert abs(st["ev_cv2"]) < 1e-6
    finally:
        e.close()


def test_writers_of_X_clear_the_energy_flags():
    r = pc.ROWS[17]
    X, massL = pc.data(r)
    e = _engine()
    flags = lambda: tuple(e.test_prep_state(want_energies=False)[k] for k in ("e0_valid", "ev_valid"))
    try:
        with pytest.raises(RuntimeError, match="status -1"):
            e.test_prep_state(want_X=True, want_energies=False)
        assert b"asb_test_prep_state" in e.lib.asb_last_error(e.h)
        e.upload(X, r.v0, r.n_loc, massL)
        with pytest.raises(RuntimeError, match="status -1"):
            e.test_prep_state()
        assert b"asb_snapshots_scale" in e.lib.asb_last_error(e.h)
        e.center(0, False)
        assert flags() == (False, False)
        e.scale(2.0)
        assert flags() == (True, True)
        e.center(1, False)                          # reads only
        assert flags() == (True, True)
        e.center(1, True)
        assert flags() == (False, False)
        e.scale(2.0)
        assert flags() == (True, True)
        e.snapshots_affine(1.0, False)
        assert flags() == (False, False)
        e.scale(1.0)
        assert flags() == (True, True)
        e.upload_rest(X, r.v0, r.n_loc, massL, 0, True)
        assert flags() == (False, False)
        e.scale(1.0)
        e.upload(X, r.v0, r.n_loc, massL)
        assert flags() == (False, False)
    finally:
        e.close()


@pytest.mark.parametrize("r", [pc.ROWS[5], pc.ROWS[-1]], ids=pc.row_id)
def test_projection_mode_starts_from_E0_bit_for_bit(r):
    X, massL = pc.data(r)
    e = _engine()
    try:
        e.upload_rest(X, r.v0, r.n_loc, massL, r.code, True)
        e.scale(0.37)
        st = e.test_prep_state()
        E0 = st["E0"]
        e.deflate_begin(2, False)                   # (the state hook wants a residual buffer: the residual mode allocates it)
        assert e.test_prep_state(want_energies=False)["e0_valid"]
        e.deflate_begin(2, False, mode=_lib.DEFLATE_PROJECT)
        assert e.deflate_stats()["energy_passes"] == 0
        assert pm.same_bits(e.test_deflate_state()["energy"], E0)
        # asb_panel_guess_stats: a guessed first panel needs more vertices than the candidate buffer holds (1536)
        me, nx, ok = e.panel_guess_stats()
        assert ok == (r.n_loc == pc.N_LARGE)
        if ok:
            assert st["mean_energy"] > 0 and st["prep_normx2"] > 0
            assert (me, nx) == (st["mean_energy"], st["prep_normx2"])
        else:
            assert (me, nx) == (0.0, 0.0)
    finally:
        e.close()


@pytest.mark.parametrize("r", [pc.ROWS[30], pc.ROWS[-1]], ids=pc.row_id)
def test_recomputed_initial_energies_lie_within_the_bound_of_E0(r, monkeypatch):
    """ASB_E0_REUSE=0 (read when the context is created, so no child process is needed): the projection mode reads X for its
    energies with k_stream<T, E2>, whose depth prep_model.depth_stream reads from the kernel; E0 has its own bound"""
    monkeypatch.setenv("ASB_E0_REUSE", "0")
    X, massL = pc.generic_data(r)
    want, _ = pm.order_tensor(X, massL, r.v0, r.n_loc, r.code, True)
    e = _engine()
    try:
        e.upload_rest(X, r.v0, r.n_loc, massL, r.code, True)
        e.scale(0.37)
        E0 = e.test_prep_state()["E0"]
        e.deflate_begin(2, False)
        e.deflate_begin(2, False, mode=_lib.DEFLATE_PROJECT)
        assert e.deflate_stats()["energy_passes"] == 1
        energy = e.test_deflate_state()["energy"]
        en = pm.ld_energies(want * 0.37)
        cfg = np.zeros(5, dtype=np.int32)
        _lib.load().asb_test_pick_cfg(pm.pad16(r.F), cfg.ctypes.data)
        assert cfg[0] == 1
        b_stream = (pm.depth_stream(int(cfg[1]), int(cfg[2])) + 2 + 1) * U * en["E0"]
        bE0 = pm.energy_bounds(en)[0]
        k = int(np.argmax(np.abs(energy - en["E0"]) - b_stream))
        assert _note("recomputed energy vs model", abs(energy[k] - en["E0"][k]), b_stream[k])
        assert (np.abs(energy - en["E0"]) <= b_stream).all() and (np.abs(energy - E0) <= b_stream + bE0).all()
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 4
def _family(name, N):
    if name == "generic":
        return pc.generic_data(pc.Row(20, N, N, 0, False, 0, True, "generic"))[0]
    if name == "offset":
        return pc.offset_data(20, N)
    return pc.translated_data(int(name[10:]), N)


def _standarize(X, rest, mass, comm=None, stream=None, quiet=True):
    """(redirect_stdout swaps sys.stdout of the whole process: thread ranks are silenced around run_ranks, not inside)"""
    from animsnapbases_amd import HipEngine, posSnapshots
    eng = HipEngine(0) if stream is None else HipEngine(0, stream=stream)
    calls, inner = [], eng.sqdev

    def counted(mu):
        calls.append(mu)
        return inner(mu)
    eng.sqdev = counted
    with contextlib.redirect_stdout(io.StringIO()) if quiet else contextlib.nullcontext():
        snaps = posSnapshots.from_arrays(X, None, rest, standarize=True, massWeight=mass is not None, engine=eng, mass=mass,
                                         comm=comm)
    return snaps, eng, len(calls)


def _psf_bound(T, code, one_sweep, n_loc, world):
    mu, var, std = pm.ld_std(T)
    sums = pm.ld_sums(T)
    F, cap = T.shape[0], _cap()
    d_rows, d_fused = pm.depth_rows(F, n_loc, cap), pm.depth_fused(F, n_loc)
    d_sum = d_fused if code == 0 else d_rows
    return std, pm.psf_rel_bound(pm.var_rel_bound(sums, mu, var, d_sum, d_fused if one_sweep else d_rows, one_sweep, world))


FAMILIES = ("generic", "offset", "translated6", "translated9", "translated13", "translated17")


@pytest.mark.parametrize("rest", ("first", "average"))
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("with_mass", (False, True))
def test_standarize_end_to_end(family, rest, with_mass):
    N = 41
    X = _family(family, N)
    mass = np.random.default_rng(11).uniform(0.25, 4.0, N) if with_mass else None
    massL = None if mass is None else np.sqrt(mass)
    code = 0 if rest == "first" else 1
    T, mean = pm.order_tensor(X, massL, 0, N, code, True)
    mu, var, _ = pm.ld_std(T)
    one_sweep = code == 0 and mu * mu <= 10 * var
    if code == 0:
        assert mu * mu <= 9 * var or mu * mu >= 11.9 * var          # no case at the threshold (exactly: test_prep_model_cpu.py)
        if family.startswith("translated") and not with_mass:
            assert one_sweep == (pc.TRANSLATED_F[int(family[10:])] == "one sweep")
    snaps, eng, n_sqdev = _standarize(X, rest, mass)
    try:
        assert n_sqdev == (0 if one_sweep else 1), "standarize() took the other branch"
        std, rel = _psf_bound(T, code, one_sweep, N, 1)
        assert _note("pre_scale_factor " + ("one sweep" if one_sweep else "second pass"), abs(float(snaps.pre_scale_factor * std - 1)), rel)
        assert pm.same_bits(eng.download_snapshots(), T * snaps.pre_scale_factor)
        assert pm.same_bits(snaps.mean, mean)
    finally:
        eng.close()


@pytest.mark.parametrize("rest,family,with_mass", (("first", "generic", True), ("average", "offset", True), ("first", "translated9", False),
                                                   ("first", "translated13", False)))
def test_standarize_on_two_thread_ranks(rest, family, with_mass):
    from thread_comm import run_ranks
    N = 41
    X = _family(family, N)
    mass = np.random.default_rng(12).uniform(0.25, 4.0, N) if with_mass else None
    massL = None if mass is None else np.sqrt(mass)
    code = 0 if rest == "first" else 1
    T, mean = pm.order_tensor(X, massL, 0, N, code, True)
    mu, var, _ = pm.ld_std(T)
    one_sweep = code == 0 and mu * mu <= 10 * var
    assert code == 1 or mu * mu <= 9 * var or mu * mu >= 11.9 * var             # no case at the threshold
    assert one_sweep == (family in ("generic", "translated9"))          # both branches run on two ranks

    def rank_fn(rank, comm):
        snaps, eng, n_sqdev = _standarize(X, rest, mass, comm=comm, stream=0, quiet=False)
        out = (snaps.pre_scale_factor, eng.v0, eng.n_loc, eng.download_snapshots(), n_sqdev, snaps.mean.copy())
        eng.close()
        return out

    with contextlib.redirect_stdout(io.StringIO()):
        outs = run_ranks(2, rank_fn)
    assert sorted(o[2] for o in outs) == [20, 21] and sum(o[2] for o in outs) == N         # an uneven split
    std, rel = _psf_bound(T, code, one_sweep, 21, 2)
    for psf, v0, n_loc, shard, n_sqdev, mean_all in outs:
        assert psf == outs[0][0]
        assert n_sqdev == (0 if one_sweep else 1)
        assert _note("pre_scale_factor two ranks", abs(float(psf * std - 1)), rel)
        assert pm.same_bits(shard, T[:, v0:v0 + n_loc] * psf)
        assert pm.same_bits(mean_all, mean)


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("r", [pc.ROWS[i] for i in (6, 15, 30, 47, 62)], ids=pc.row_id)
def test_heldout_preparation_of_the_training_frames(r):
    assert r.mass and r.subtract            # x m - mean: the one place where a contraction can change a bit
    X, massL = pc.generic_data(r)
    a = 0.37
    e = _engine()
    try:
        e.upload_rest(X, r.v0, r.n_loc, massL, r.code, r.subtract)
        mean = e.get_mean()
        e.scale(a)
        train = e.download_snapshots()
        e.heldout_upload(X, massL, r.subtract, a)
        rows, owned = e.rows_gather(1, np.arange(r.v0, r.v0 + r.n_loc))
        assert owned.all()
        held = rows.transpose(1, 0, 2)
        mx = X[:, r.v0:r.v0 + r.n_loc] * (1.0 if massL is None else massL[r.v0:r.v0 + r.n_loc, None])
        bound = 2 * 2.0 ** -52 * (np.abs(mx) + (np.abs(mean)[None] if r.subtract else 0.0)) * abs(a)
        diff = np.abs(held - train)
        k = int(np.argmax(diff - bound))
        assert _note("held-out vs training", diff.ravel()[k], bound.ravel()[k])
        assert (diff <= bound).all()
        print("  held-out entries that differ from the training tensor in the last bits: %d of %d (contraction in k_heldout_prep)"
              % (int((held != train).sum()), held.size))
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 6
def test_download_of_700000_vertices():
    """3 n_loc = 2 100 000 rows are 65 625 strips of 32: more than grid.y holds; asb_download_vertex_major puts them on grid.x"""
    n = 700000
    assert (3 * n + 31) // 32 > 65535
    X = np.random.default_rng(6).integers(-1000, 1001, size=(1, n, 3)).astype(np.float64)
    e = _engine()
    try:
        e.upload(X, 0, n)
        assert np.array_equal(e.download_snapshots(), X)
        e.deflate_begin(1, False)
        assert np.array_equal(e.download_residual(), X)
    finally:
        e.close()


def test_zz_observed():
    """Checks nothing: every achieved / bound is asserted where it is measured (_note).  This only prints the largest ratio per
    group that the tests of this process have seen so far (all of them in a whole run of the file, fewer under -k or with the
    file split over workers); the OBSERVED table above is a copy of one whole run."""
    for g in sorted(_SEEN):
        print("OBSERVED-MAX %-40s %.3f" % (g, _SEEN[g]))
