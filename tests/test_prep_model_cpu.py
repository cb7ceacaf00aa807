"""CPU: the model and the case table behind test_gpu_prep.py, and both branches of posSnapshots.standarize() on a CPU double of
the engine that offers the fused upload.

 * the float64 order model reproduces the oracle's preparation (tensor, rest shape, pre_scale_factor) on the small rows;
 * the longdouble model stays in its type;
 * every edge of prep_cases.EDGES occurs in some row with both rest shapes and with and without massL; the integer rows fit 53 bits;
 * every translated case lies on its side of the mu^2 > 10 var threshold (ratio <= 9, or >= 12 up to the relative F sigma^2 / d^2 = 1.3e-9
   that the noise adds to var: without noise the ratio at F = 13 is F - 1 = 12 exactly, and noise can only lower it);
 * standarize() takes the one-sweep branch and the second pass as predicted (a counter on `sqdev`), and pre_scale_factor lies
   within its bound of longdouble 1 / std.  The double sums with NumPy's pairwise sum: 128-term chains, then a tree, depth < 64.
"""
import numpy as np
import pytest

import prep_cases as pc
import prep_model as pm
from fake_engine import FakeEngine
from oracle import asb_oracle as orc

U = pm.U
SMALL = [r for r in pc.ROWS if r.F * r.n_loc <= 4000]


class FusedFakeEngine(FakeEngine):
    """FakeEngine plus the fused upload of HipEngine.upload_rest: (sum(x), sum(x^2) where one sweep has it: rest shape 0)"""

    def __init__(self):
        FakeEngine.__init__(self)
        self.n_sqdev = 0

    def upload_rest(self, X, v0, n_loc, massL, code, subtract):
        self.upload(X, v0, n_loc, massL)
        s = self.center(code, subtract)
        return s, (float((self.X ** 2).sum()) if code == 0 else None)

    def sqdev(self, mu):
        self.n_sqdev += 1
        return FakeEngine.sqdev(self, mu)


@pytest.mark.parametrize("r", SMALL, ids=pc.row_id)
def test_order_model_reproduces_the_oracle(r):
    X, massL = pc.data(r)
    if r.N != r.n_loc:          # the oracle has no shards: the shard as a tensor of its own
        X, massL = X[:, r.v0:r.v0 + r.n_loc], None if massL is None else massL[r.v0:r.v0 + r.n_loc]
    Y, mean = pm.order_tensor(X, massL, 0, r.n_loc, r.code, r.subtract)
    ref = orc.prepare_snapshots(X, "first" if r.code == 0 else "average", False, massL)
    scaled = X if massL is None else X * massL[:, None]
    if r.code == 0:
        assert pm.same_bits(mean, ref["mean"])
    else:               # a mean is a sum and the oracle's has another order: F roundings of sum |x| / F
        assert (np.abs(mean - ref["mean"]) <= (r.F + 2) * U * np.abs(scaled).sum(axis=0) / r.F).all()
    if r.subtract:
        want = ref["snapTensor"] - ref["mean"][None]
        tol = 0.0 if r.code == 0 else np.abs(mean - ref["mean"])[None] + U * (np.abs(want) + np.abs(Y))
        assert (np.abs(Y - want) <= tol).all()
        if r.F * r.n_loc > 1 and np.std(want) > 0:
            full = orc.prepare_snapshots(X, "first" if r.code == 0 else "average", True, massL)
            mu, var, std = pm.ld_std(Y)
            sums = pm.ld_sums(Y)
            rel = pm.psf_rel_bound(pm.var_rel_bound(sums, mu, var, 64, 64, False)) + float(2 * np.abs(Y - want).max() / std)
            assert abs(full["pre_scale_factor"] * std - 1) <= rel
    else:
        assert pm.same_bits(Y, ref["snapTensor"])


def test_longdouble_model_stays_in_its_type():
    r = pc.ROWS[9]
    X, massL = pc.generic_data(r)
    for code in (0, 1):
        Y, mean = pm.ld_prepare(X, massL, r.v0, r.n_loc, code, True)
        assert Y.dtype == pm.LD and mean.dtype == pm.LD
        T, _ = pm.order_tensor(X, massL, r.v0, r.n_loc, code, True)
        s = pm.ld_sums(T, 0.25)
        assert all(s[k].dtype == pm.LD for k in ("sum", "abs", "sq", "sqdev"))
        en = pm.ld_energies(T)
        assert all(en[k].dtype == pm.LD for k in ("E0", "s", "A", "mv", "EV"))
        assert all(b.dtype == pm.LD for b in pm.energy_bounds(en))
        assert all(v.dtype == pm.LD for v in pm.ld_std(T))
        # and it is the same preparation: the float64 tensor lies within its elementwise roundings of it
        assert (np.abs(T.astype(pm.LD) - Y) <= 3 * U * (np.abs(Y) + np.abs(mean)[None]) + r.F * U * np.abs(mean)[None]).all()
    assert np.finfo(pm.LD).eps < 2.0 ** -60, "numpy.longdouble is no wider than float64 here"


def test_lane_sum_is_the_wave_sum_of_the_ingest_test_below_65_frames_and_a_chain_above():
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((5, 64))
    assert pm.same_bits(pm.lane_sum(rows[:, :17]), pm.wave_sum64(np.pad(rows[:, :17], ((0, 0), (0, 47)))))
    big = rng.standard_normal((3, 130))
    v = np.zeros((3, 64))
    for f in range(130):        # lane f % 64 adds its entries in increasing f
        v[:, f % 64] = v[:, f % 64] + big[:, f]
    assert pm.same_bits(pm.lane_sum(big), pm.wave_sum64(v))


def test_every_edge_is_covered_with_both_rest_shapes_and_with_and_without_mass():
    assert 55 <= len(pc.ROWS) <= 75
    for name, pred in pc.EDGES.items():
        hit = {(r.code, r.mass) for r in pc.ROWS if pred(r)}
        assert hit == {(0, False), (0, True), (1, False), (1, True)}, (name, hit)
    for code in (0, 1):
        assert {r.subtract for r in pc.ROWS if r.code == code} == {False, True}
        assert {r.family for r in pc.ROWS if r.code == code} == {"integer", "generic"}
    assert {r.F for r in pc.ROWS if r.n_loc == pc.N_LARGE} == set(pc.F_LARGE)
    assert {pm.pad16(r.F) - r.F for r in pc.ROWS} >= {0, 1, 14, 15}
    assert {3 * r.n_loc for r in pc.ROWS} >= {3, 6, 30, 33, 63, 66, 129, 1026}
    for cap in (256, 2048, 2432):       # the facts the GPU file asserts from the real cap hold for the caps of gfx950 parts
        facts = pc.large_grid_facts(cap)
        assert all(facts.values()) or cap == 256, (cap, facts)


@pytest.mark.parametrize("r", [r for r in pc.ROWS if r.family == "integer"], ids=pc.row_id)
def test_integer_rows_fit_53_bits(r):
    X, massL = pc.integer_data(r)
    for a in (1.0, 4.0):
        T, mean = pm.order_tensor(X, massL, r.v0, r.n_loc, r.code, r.subtract)
        assert (mean == np.rint(mean)).all()
        assert pm.fits53(T * a)
        pm.ev_integer_model(T * a)          # asserts E0 and sum_d s_d^2 below 2^53
        E0 = pm.ld_energies(T * a)["E0"]
        assert float(E0.sum()) < 2.0 ** 53


@pytest.mark.parametrize("F", sorted(pc.TRANSLATED_F))
def test_translated_cases_lie_on_their_side_of_the_threshold(F):
    d, sigma = 100.0, 1e-3
    X = pc.translated_data(F, 40, d, sigma)
    T, _ = pm.order_tensor(X, None, 0, 40, 0, True)
    mu, var, _ = pm.ld_std(T)
    ratio = mu * mu / var
    print("F = %d: mu^2 / var = %.12f" % (F, float(ratio)))
    assert abs(float(ratio) - (F - 1)) <= 2 * F * (F - 1) * sigma ** 2 / d ** 2
    if pc.TRANSLATED_F[F] == "one sweep":
        assert ratio <= 9
    else:
        assert ratio >= 12 * (1 - 2 * F * sigma ** 2 / d ** 2)


def _standarize_on_the_double(X, rest, mass):
    from animsnapbases_amd import posSnapshots
    eng = FusedFakeEngine()
    snaps = posSnapshots.from_arrays(X, None, rest, standarize=True, massWeight=mass is not None, engine=eng, mass=mass)
    return snaps, eng


@pytest.mark.parametrize("rest", ("first", "average"))
@pytest.mark.parametrize("family", ("generic", "offset", "translated6", "translated9", "translated13", "translated17"))
@pytest.mark.parametrize("with_mass", (False, True))
def test_standarize_takes_the_predicted_branch_and_lands_within_the_bound(family, rest, with_mass):
    N = 40
    rng = np.random.default_rng(11)
    if family == "generic":
        X = pc.generic_data(pc.Row(20, N, N, 0, False, 0, True, "generic"))[0]
    elif family == "offset":
        X = pc.offset_data(20, N)
    else:
        X = pc.translated_data(int(family[10:]), N)
    mass = rng.uniform(0.25, 4.0, N) if with_mass else None
    massL = None if mass is None else np.sqrt(mass)
    code = 0 if rest == "first" else 1
    snaps, eng = _standarize_on_the_double(X, rest, mass)
    T, mean = pm.order_tensor(X, massL, 0, N, code, True)
    mu, var, std = pm.ld_std(T)
    one_sweep = code == 0 and mu * mu <= 10 * var
    assert code == 1 or mu * mu <= 9 * var or mu * mu >= 11.9 * var             # no case at the threshold
    if family.startswith("translated") and code == 0 and not with_mass:
        assert one_sweep == (pc.TRANSLATED_F[int(family[10:])] == "one sweep")
    assert eng.n_sqdev == (0 if one_sweep else 1), "standarize() took the other branch"
    sums = pm.ld_sums(T)
    # (the double's own mean of rest shape 1 is np.mean, not the lane order: its tensor differs from T by that much)
    dT = np.abs(eng.X / snaps.pre_scale_factor - T).max() if code == 1 else 0.0
    rel = pm.psf_rel_bound(pm.var_rel_bound(sums, mu, var, 64, 64, one_sweep)) + float(2 * dT / std)
    got = abs(float(snaps.pre_scale_factor * std - 1))
    print("%s %s mass=%s: %s, |psf std - 1| = %.3e of bound %.3e" % (family, rest, with_mass, "one sweep" if one_sweep else "second pass", got, rel))
    assert got <= rel


def test_both_branches_were_taken():
    taken = set()
    for F in (6, 17):
        snaps, eng = _standarize_on_the_double(pc.translated_data(F, 40), "first", None)
        taken.add(eng.n_sqdev)
    assert taken == {0, 1}
    # the plain double (no fused upload) always takes the second pass: fake_engine.py is unchanged
    assert not hasattr(FakeEngine, "upload_rest")
