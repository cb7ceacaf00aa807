"""GPU (-m gpu): the interpolation-point kernels of csrc/asb_pod.hip -- k_deim_residual, k_deim_solve, k_deim_pick, the block
residuals, the S^T row energies (one shard and own rows + halo), the halo pack / fill, k_sum_all and the host arg-max folds --
each through the HipEngine call that launches it, against tests/deim_model.py (numpy.longdouble) at the shapes of
tests/deim_cases.py: every slice / stride / grid-cap branch, ties in every placement, shards, degenerate bases.

Bounds.  Energies and largest |r| follow the dot-product bound of deim_model.bound: 8 (T + 4) 2^-53 sum|terms| with the T of
the kernel's chain; an index is compared after asserting that the model's two best energies are further apart than that.
The `maxabs` of a whole deim_run depends on the conditioning of the k x k systems.  Its tolerance is 16 times the largest
relative deviation of the float64 from-scratch loop (numpy.linalg.solve, the reference's arithmetic) from the longdouble
model on the same case -- the bordered inverse accumulates over k steps what a fresh solve does not -- and no less than
16 * 2^-52, which the measurement cannot resolve.  Measured (tests/deim_cases.py run as a program; n = K + 100, seed = n):

    K     smallest relative gap   float64 loop's largest relative deviation of maxabs
    1     2.45e-03                0.00e+00
    2     1.87e-01                3.77e-17
    3     7.79e-02                5.73e-17
    130   1.15e-03                6.71e-14
    256   6.42e-04                1.34e-12
    257   1.62e-03                4.79e-13
    300   4.32e-04                2.19e-12
    552   1.92e-04                6.22e-12
    553   1.55e-04                2.00e-10
    600   8.97e-05                2.99e-12

Defect found by this bound: with coef = Minv b alone the device's maxabs at K = 257 deviated by 1.57e-11 against the
tolerance 16 * 4.79e-13 = 7.67e-12 (Pt right, solve_failed 0) -- the bordered inverse keeps the rounding of every earlier
step.  k_deim_solve now refines coef once by its own residual.
"""
import contextlib
import functools
import io

import numpy as np
import pytest

import deim_cases as dc
import deim_model as dm

pytestmark = pytest.mark.gpu

LD = np.longdouble
DEFLATE_RESIDUAL = 0


def _basis_engine(comps, v0=0, N=None):
    """an engine holding rows [v0, v0 + n) of N with `comps` (K, n, 3) as its basis"""
    from animsnapbases_amd import HipEngine
    n = comps.shape[1]
    e = HipEngine(0)
    e.upload(np.zeros((4, n if N is None else N, 3)), v0, n)
    e.components_upload(comps)
    return e


def _residual_engine(X, v0=0, n_loc=None):
    """an engine in the residual mode; what it holds as the residual (F, n_loc, 3)"""
    from animsnapbases_amd import HipEngine, _lib
    e = HipEngine(0)
    e.upload(X, v0, X.shape[1] if n_loc is None else n_loc)
    e.deflate_begin(1, False, mode=_lib.DEFLATE_RESIDUAL)
    return e, e.download_residual()


def _rows_of(R):
    """(F, n, 3) -> (n, 3 F): the row of constraint j, x, y, z sub-rows"""
    return np.ascontiguousarray(R.transpose(1, 2, 0)).reshape(R.shape[1], 3 * R.shape[0])


def _separated(s):
    assert float(s["val"] - s["second"]) > 2 * float(np.max(s["ebound"])), "the case does not separate its two best rows"


# ---- (a) deim_step ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K,k,v0,N", dc.STEP_CASES)
def test_deim_step_energy_and_index(n, K, k, v0, N):
    comps, coef = dc.step_inputs(n, K, k)
    s = dm.step(comps, k, coef)
    e = _basis_engine(comps, v0, N)
    idx, val = e.deim_step(k, coef)
    print("deim_step n %d k %d: |dev - model| %.2e, bound %.2e" % (n, k, abs(float(LD(val) - s["val"])), s["ebound"][s["idx"]]))
    if n > 1:
        _separated(s)
    assert idx == v0 + s["idx"]
    assert abs(float(LD(val) - s["val"])) <= s["ebound"][s["idx"]]


# ---- (b) ties -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,rows", dc.TIE_CASES)
def test_ties_take_the_lowest_index(name, n, rows):
    comps = dc.tie_basis(n, rows)
    e = _basis_engine(comps)
    for k, coef in ((0, None), (1, np.full((3, 1), 0.5))):
        idx, val = e.deim_step(k, coef)
        s = dm.step(comps, k, coef)
        assert idx == min(rows) and abs(float(LD(val) - s["val"])) <= s["ebound"][idx], (name, k)
    Pt, maxabs, bad = e.deim_run()                    # (k_deim_pick folds the same partials on the device)
    assert bad == 0 and Pt[0] == min(rows) and Pt[1] not in rows and 0 <= Pt[1] < n
    for p in (1, 2):
        blk = dc.tie_block_basis(n, p, rows)
        eb = _basis_engine(blk)
        assert eb.deim_block_step(0, p, None, 1)[0] == min(rows) * p, (name, p)
        assert eb.deim_block_step(0, p, None, p)[0] == min(rows), (name, p)
        eb.close()
    e.close()


@functools.lru_cache(maxsize=None)
def _st_big(n_rows):
    return dc.st_matrix(n_rows, dc.ST_COLS, n_rows, per_row=5, long_row=False)


@pytest.mark.parametrize("n_rows,rows", [(1000, (5, 40)), (1000, (10, 200)), (1000, (100, 300, 700)), (65536 + 300, (300, 65536 + 5))])
def test_st_ties_take_the_lowest_vertex(n_rows, rows):
    St = dc.st_tie(_st_big(n_rows), rows)
    e, R = _residual_engine(np.random.default_rng(7).normal(size=(16, dc.ST_COLS, 3)))
    m = dm.st_rows(St.indptr, St.indices, St.data, _rows_of(R))
    assert np.flatnonzero(m["energy"] == m["energy"].max()).tolist() == sorted(rows)
    assert float(m["energy"].max() - np.delete(m["energy"], list(rows)).max()) > 2 * m["ebound"].max()
    e.st_upload(St)
    v, val = e.st_residual_argmax()
    assert v == min(rows) and abs(float(LD(val) - m["energy"][v])) <= m["ebound"][v]


# ---- (c) deim_block_step ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p,k", dc.BLOCK_CASES)
def test_deim_block_step(n, p, k):
    comps, coef = dc.block_inputs(n, p, k)
    e = _basis_engine(comps)
    for group in sorted({1, p}):
        s = dm.block_step(comps, k, p, coef, group)
        idx, val, am = e.deim_block_step(k, p, coef, group)
        if n > group:
            _separated(s)
        assert idx == s["idx"], (group,)
        assert abs(float(LD(val) - s["val"])) <= s["ebound"][s["idx"]], (group,)
        assert abs(float(LD(am) - s["maxabs"])) <= s["abound"], (group,)


# ---- (d) deim_run -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_runs():
    return dc.run_golden()


@pytest.mark.parametrize("K", sorted(dc.RUN_SEEDS))
def test_deim_run_against_the_from_scratch_model(K, golden_runs):
    g = golden_runs[K]
    assert g["gap"].min() > dc.RUN_GAP                 # (tests/test_deim_model_cpu.py recomputes the table)
    comps = dc.run_basis(K)
    e = _basis_engine(comps)
    Pt, maxabs, bad = e.deim_run()
    tol = 16 * max(g["dev64"], 2.0 ** -52)
    dev = float(np.max(np.abs(maxabs - g["maxabs"]) / g["maxabs"]))
    print("deim_run K %d: maxabs deviates by %.2e (tolerance %.2e, float64 from-scratch loop %.2e)" % (K, dev, tol, g["dev64"]))
    assert bad == 0
    assert Pt.tolist() == g["Pt"].tolist() and len(set(Pt.tolist())) == K
    assert np.isfinite(maxabs).all() and dev <= tol
    if K == 130:
        for m in (0, 57, K - 1):
            assert np.array_equal(e.deim_row(int(Pt[m])), comps[:, Pt[m], :])


# ---- (e) degenerate bases ----------------------------------------------------------------------------------------------------
def _degenerate(which):
    comps = dc.run_basis(3)
    comps = np.concatenate([comps, dc.run_basis(3, seed=9)[:1]])               # K = 4, n = 103
    if which == "dependent":
        comps[1] = 2 * comps[0]
    else:
        comps[0, :, 1] = 0.0
    return comps


@pytest.mark.parametrize("which", ["dependent", "zero_dimension"])
def test_deim_run_on_a_degenerate_basis_stays_in_range(which):
    comps = _degenerate(which)
    e = _basis_engine(comps)
    Pt, maxabs, bad = e.deim_run()
    assert np.all((Pt >= 0) & (Pt < comps.shape[1])) and not np.isnan(maxabs).any()
    if which == "dependent":
        assert maxabs[1] <= 1e-12 * np.abs(comps).max() or bad != 0
    else:
        assert bad != 0                                                           # m00 == 0 in dimension 1


@pytest.mark.parametrize("which", ["dependent", "zero_dimension"])
def test_deim_of_a_degenerate_basis_equals_the_host_loop(which, tmp_path, monkeypatch):
    from test_gpu_blocks_deim import _build
    comps = _degenerate(which)
    K, n = comps.shape[0], comps.shape[1]
    ns, cc = _build(np.random.default_rng(3).normal(size=(K + 4, n, 3)), K, tmp_path, "deim", "pod_vectorized", 1)

    def run():
        ns._engine.components_upload(comps)
        cc._comps, cc._comps_on_device, cc.numComp = None, True, K
        cc.geom_Pt = None
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            cc.deim()
        return (None if cc.geom_Pt is None else cc.geom_Pt.tolist()), "ERROR!: zero residual!!" in buf.getvalue()
    dev = run()
    monkeypatch.setenv("ASB_DEIM", "host")
    host = run()
    assert dev == host
    assert dev[1] == (which == "dependent")


# ---- (f) S^T row energies, one shard -------------------------------------------------------------------------------------------
def _st_single_checks(St, F, seed, blocks=True):
    n = St.shape[1]
    rng = np.random.default_rng(seed)
    e, R = _residual_engine(rng.normal(size=(F, n, 3)))
    M = _rows_of(R)
    e.st_upload(St)
    m = dm.st_rows(St.indptr, St.indices, St.data, M)
    i, best, second = dm.first_argmax(m["energy"])
    v, val = e.st_residual_argmax()
    if St.shape[0] > 1:
        assert float(best - second) > 2 * m["ebound"].max()
    assert v == i and abs(float(LD(val) - best)) <= m["ebound"][i]
    # |R|^2: row sums of 3 F squares, then n / 1024 additions per thread and the block sum
    tot = (M.astype(LD) ** 2).sum()
    assert abs(float(LD(e.residual_norm2()) - tot)) <= dm.bound(3 * F + n // 1024 + 16, float(tot))
    if not blocks:
        return
    for p in (1, 2):
        k = 1
        comps, coef = rng.normal(size=((k + 1) * p, n, 3)), rng.normal(size=(3, k * p, p))
        e.components_upload(comps)
        r, S = dm.block_residual(comps, k, p, coef)
        mb = dm.st_rows(St.indptr, St.indices, St.data, r.reshape(n, 3 * p), S.reshape(n, 3 * p), extra_terms=k * p + 1)
        i, best, second = dm.first_argmax(mb["energy"])
        v, val, am = e.deim_block_step_st(k, p, coef)
        if St.shape[0] > 1:
            assert float(best - second) > 2 * mb["ebound"].max()
        assert v == i and abs(float(LD(val) - best)) <= mb["ebound"][i], p
        assert abs(float(LD(am) - mb["amax"].max())) <= mb["abound"].max(), p


@pytest.mark.parametrize("F", dc.ST_F)
@pytest.mark.parametrize("n_rows", dc.ST_ROWS)
def test_st_row_energies(n_rows, F):
    _st_single_checks(dc.st_matrix(n_rows, dc.ST_COLS, 100 * n_rows + F), F, n_rows + F)


@pytest.mark.parametrize("which", ["grid cap", "arg-max stride"])
def test_st_row_energies_many_rows(which):
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n_rows = 8 * n_cu * 4 + 5 if which == "grid cap" else 65536 + 300
    _st_single_checks(_st_big(n_rows), 16, n_rows)


# ---- (g) S^T over own rows and halo, in one process ------------------------------------------------------------------------------
SHARDS = [(0, 21), (21, 20), (41, 20)]
N_SH = 61


def _sharded_matrix():
    """every vertex is owned by rank 0 or rank 2 (rank 1 owns nothing, rank 2 has no halo)"""
    A = dc.st_matrix(200, N_SH, 23).tolil()
    for v in range(200):
        cols = A.rows[v]
        if cols and 21 <= cols[0] < 41:
            A[v, v % 21] = 0.75
    out = A.tocsr()
    out.sort_indices()
    return out


def _dev_rows(rows2d):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rows2d)).cuda()


@pytest.mark.parametrize("rank", [0, 1, 2])
def test_st_shard_equals_the_single_shard_bit_for_bit(rank):
    from scipy import sparse
    from animsnapbases_amd.constraints import st_shard_plan
    St = _sharded_matrix()
    F, k, p = 90, 1, 2
    rng = np.random.default_rng(31)
    X = rng.normal(size=(F, N_SH, 3))
    comps, coef = rng.normal(size=((k + 1) * p, N_SH, 3)), rng.normal(size=(3, k * p, p))
    pl = st_shard_plan(St, SHARDS, rank)
    v0, n = SHARDS[rank]
    h = len(pl["halo"])
    assert (rank, len(pl["owned"]) > 0, h > 0) in ((0, True, True), (1, False, False), (2, True, False))
    A, RA = _residual_engine(X)
    B, RB = _residual_engine(X, v0, n)
    assert np.array_equal(RB, RA[:, v0:v0 + n])
    A.components_upload(comps)
    B.components_upload(comps[:, v0:v0 + n])
    B.st_upload_shard(pl["indptr"], pl["slots"], pl["data"], h)
    Fp = (B.xchg_len() - 2) // 3
    # the halo rows, laid out as the owner packs them, in a permuted order
    perm = np.random.default_rng(rank).permutation(h)
    src0 = np.zeros((max(h, 1), 3, Fp))
    src1 = np.zeros((max(h, 1), comps.shape[0], 3))
    if h:
        src0[perm, :, :F] = RA[:, pl["halo"], :].transpose(1, 2, 0)
        src1[perm] = comps[:, pl["halo"], :].transpose(1, 0, 2)
    t0, t1 = _dev_rows(src0.reshape(max(h, 1), -1)), _dev_rows(src1.reshape(max(h, 1), -1))
    B.st_halo_fill(0, t0.data_ptr(), perm, max(h, 1))
    B.st_halo_fill(1, t1.data_ptr(), perm, max(h, 1))
    assert np.array_equal(B.st_halo_download(0), RA[:, pl["halo"], :].transpose(1, 2, 0))
    assert np.array_equal(B.st_halo_download(1), comps[:, pl["halo"], :])
    got_r = B.st_shard_residual_argmax()
    got_b = B.deim_block_step_st_shard(k, p, coef)
    if not len(pl["owned"]):
        assert got_r == (-1, -1.0) and got_b[:2] == (-1, -1.0) and got_b[2] == 0.0
        return
    # the one-shard engine on the same global data, with the rows of other owners emptied
    mask = np.zeros(St.shape[0])
    mask[pl["owned"]] = 1.0
    St_r = (sparse.diags(mask) @ St).tocsr()
    St_r.eliminate_zeros()
    A.st_upload(St_r)
    ref_r = A.st_residual_argmax()
    ref_b = A.deim_block_step_st(k, p, coef)
    assert (int(pl["owned"][got_r[0]]), got_r[1]) == ref_r
    assert (int(pl["owned"][got_b[0]]), got_b[1], got_b[2]) == ref_b
    # and the model, through the split form
    m = dm.st_rows_split(pl["indptr"], pl["slots"], pl["data"], _rows_of(RB), _rows_of(RA[:, pl["halo"], :]))
    i = dm.first_argmax(m["energy"])[0]
    assert got_r[0] == i and abs(float(LD(got_r[1]) - m["energy"][i])) <= m["ebound"][i]
    r, S = dm.block_residual(comps, k, p, coef)
    r, S = r.reshape(N_SH, 3 * p), S.reshape(N_SH, 3 * p)
    mb = dm.st_rows_split(pl["indptr"], pl["slots"], pl["data"], r[v0:v0 + n], r[pl["halo"]], S[v0:v0 + n], S[pl["halo"]],
                          extra_terms=k * p + 1)
    i = dm.first_argmax(mb["energy"])[0]
    assert got_b[0] == i and abs(float(LD(got_b[1]) - mb["energy"][i])) <= mb["ebound"][i]
    assert abs(float(LD(got_b[2]) - mb["amax"].max())) <= mb["abound"].max()


@pytest.mark.parametrize("h", [0, 1, 7])
def test_halo_pack_fill_download_round_trip(h):
    import torch
    F, K, v0, n = 90, 5, 21, 20
    rng = np.random.default_rng(h)
    X, comps = rng.normal(size=(F, N_SH, 3)), rng.normal(size=(K, n, 3))
    B, RB = _residual_engine(X, v0, n)
    B.components_upload(comps)
    B.st_upload_shard(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0), h)
    Fp = (B.xchg_len() - 2) // 3
    gidx = v0 + rng.permutation(n)[:max(h, 1) + 2]                      # rows of this shard, any order
    slot = rng.permutation(len(gidx))[:h]                               # halo slot s <- packed row slot[s]
    for which, length in ((0, 3 * Fp), (1, 3 * K)):
        out = torch.full((len(gidx), length), -7.0, dtype=torch.float64, device="cuda")
        B.st_halo_pack(which, gidx, out.data_ptr())
        packed = out.cpu().numpy()
        if which == 0:
            want = np.zeros((len(gidx), 3, Fp))
            want[:, :, :F] = RB[:, gidx - v0, :].transpose(1, 2, 0)
            assert np.array_equal(packed, want.reshape(len(gidx), -1))
        else:
            assert np.array_equal(packed, comps[:, gidx - v0, :].transpose(1, 0, 2).reshape(len(gidx), -1))
        B.st_halo_fill(which, out.data_ptr(), slot, len(gidx))
        got = B.st_halo_download(which)
        rows = (gidx - v0)[slot]
        assert np.array_equal(got, RB[:, rows, :].transpose(1, 2, 0) if which == 0 else comps[:, rows, :])


def test_st_shard_row_with_alternating_own_and_halo_slots():
    F, v0, n, h = 16, 21, 20, 3
    rng = np.random.default_rng(12)
    X = rng.normal(size=(F, N_SH, 3))
    B, RB = _residual_engine(X, v0, n)
    Fp = (B.xchg_len() - 2) // 3
    indptr = np.array([0, 6, 6, 9], dtype=np.int64)
    slots = np.array([0, n, 1, n + 1, 19, n + 2, n, n + 2, 5], dtype=np.int64)      # own, halo, own, halo, ...; empty; halo first
    data = rng.uniform(-1.5, 1.5, size=9)
    halo_rows = np.array([2, 47, 60])
    B.st_upload_shard(indptr, slots, data, h)
    src = np.zeros((h, 3, Fp))
    src[:, :, :F] = X[:, halo_rows, :].transpose(1, 2, 0)
    t = _dev_rows(src.reshape(h, -1))
    B.st_halo_fill(0, t.data_ptr(), np.arange(h), h)
    m = dm.st_rows_split(indptr, slots, data, _rows_of(RB), _rows_of(X[:, halo_rows, :]))
    i, best, second = dm.first_argmax(m["energy"])
    assert float(best - second) > 2 * m["ebound"].max()
    v, val = B.st_shard_residual_argmax()
    assert v == i and abs(float(LD(val) - best)) <= m["ebound"][i]


# ---- a basis beyond the solve kernel's LDS is refused on the host ------------------------------------------------------------------
def test_deim_run_refuses_a_basis_beyond_the_lds_before_any_launch():
    import torch
    lds = torch.cuda.get_device_properties(0).shared_memory_per_block
    K = (lds // 8 - 64) // 11 + 1                     # the first K whose (11 K + 64) doubles do not fit
    comps = np.random.default_rng(1).normal(size=(K, K, 3))
    e = _basis_engine(comps)
    e.sync()
    e.prof_reset(True)
    assert e.deim_run() is None
    assert e.prof_get()[0] == 0
    assert "LDS" in e.lib.asb_last_error(e.h).decode()
