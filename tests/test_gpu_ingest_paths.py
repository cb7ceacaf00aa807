"""GPU (-m gpu): the four snapshot ingest calls -- asb_snapshots_upload, _upload_rest, _adopt_dev, _adopt_dev_rest -- give the
same prepared tensor and the same rest shape, bit for bit, and both equal a NumPy model to the last bit.

The model is what posSnapshots.do_snapshots_precomputations documents: the shard [v0, v0 + n_loc) of the (F, N, 3) animation,
every vertex scaled by massL, then the rest shape (code 0: the first frame; code 1: the mean over the frames) taken from the
SCALED tensor and, with `subtract`, taken off every frame: m x_f - m x_0, one multiply and at most one subtract per element, so
there is nothing to tolerate.  The mean of code 1 is a sum, and a sum has an order: k_center gives each of the F <= 64 frames
of a row to one lane of a wave and adds the lanes in an xor butterfly over the distances 32, 16, 8, 4, 2, 1; the model adds in
that order (_wave_sum) and divides by F.

The sums the calls return -- sum(x), and sum(x^2) where the fused call computes it -- are compared with numpy.longdouble sums of
the model: at most 3 * 7 * 17 = 357 terms added in some tree order, every partial sum bounded by sum |term|, so the error is
below 357 * 2^-53 * sum |term|; the squares carry one more rounding each.  64 * 2^-53 * sum |term| would already cover a
balanced tree many times over; the bound used is that one.

F = 5 and 17 (neither a multiple of the 16-frame padding), N = 7 vertices, the whole range and the shard v0 = 2, n_loc = 3.
The host calls get the whole (F, N, 3) array and the global massL; the device calls a torch tensor of the shard and massL of
the shard.
"""
import itertools

import numpy as np
import pytest

from animsnapbases_amd import _lib

pytestmark = pytest.mark.gpu

N = 7
U = 2.0 ** -53
PATHS = ("host", "host_fused", "device", "device_fused")


def _inputs(F):
    rng = np.random.default_rng(1000 + F)
    X = rng.standard_normal((F, N, 3)) + 3.0 * rng.standard_normal((1, N, 3))
    massL = rng.uniform(0.5, 2.0, N)
    return X, massL


def _wave_sum(rows):
    """(R, F <= 64) -> (R): lane f holds 0 + rows[:, f], then the xor butterfly of wave_sum (every lane ends with the same value)"""
    v = np.zeros((rows.shape[0], 64))
    v[:, :rows.shape[1]] = rows
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    assert (v == v[:, :1]).all()
    return v[:, 0]


def _model(X, massL, v0, n_loc, code, subtract):
    F = X.shape[0]
    Y = X[:, v0:v0 + n_loc].copy()
    if massL is not None:
        Y = Y * massL[v0:v0 + n_loc, None]
    if code == 0:
        mean = Y[0].copy()
    else:
        mean = (_wave_sum(Y.reshape(F, n_loc * 3).T.copy()) / float(F)).reshape(n_loc, 3)
    if subtract:
        Y = Y - mean[None]
    return Y, mean


def _ingest(path, X, massL, v0, n_loc, code, subtract):
    """-> (tensor, mean, sum, sum of squares or None) of one ingest path on a fresh engine"""
    import torch
    from animsnapbases_amd import HipEngine
    F = X.shape[0]
    e = HipEngine(0)
    try:
        if path.startswith("device"):
            shard = torch.from_numpy(np.ascontiguousarray(X[:, v0:v0 + n_loc])).to("cuda:0")
            torch.cuda.synchronize()
            m_loc = None if massL is None else massL[v0:v0 + n_loc]
        if path == "host":
            e.upload(X, v0, n_loc, massL)
            s, s2 = e.center(code, subtract), None
        elif path == "host_fused":
            s, s2 = e.upload_rest(X, v0, n_loc, massL, code, subtract)
        elif path == "device":
            e.adopt_device(shard.data_ptr(), F, n_loc, m_loc, v0, N)
            s, s2 = e.center(code, subtract), None
        else:
            s, s2 = e.adopt_device_rest(shard.data_ptr(), F, n_loc, m_loc, v0, N, code, subtract)
        return e.download_snapshots(), e.get_mean(), s, s2
    finally:
        e.close()


def _same_bits(a, b):
    return a.shape == b.shape and (a.view(np.uint64) == b.view(np.uint64)).all()


CASES = list(itertools.product((5, 17), ((0, N), (2, 3)), (False, True), (0, 1), (False, True)))


@pytest.mark.parametrize("F,shard,with_mass,code,subtract", CASES)
def test_four_ingest_paths_agree_bitwise_and_match_the_model(F, shard, with_mass, code, subtract):
    v0, n_loc = shard
    X, massL = _inputs(F)
    if not with_mass:
        massL = None
    want, want_mean = _model(X, massL, v0, n_loc, code, subtract)
    big = want.astype(np.longdouble)
    sum_ref, abs_ref = big.sum(), np.abs(big).sum()
    sq_ref = (big * big).sum()
    got = {p: _ingest(p, X, massL, v0, n_loc, code, subtract) for p in PATHS}
    for p in PATHS:
        T, mean, s, s2 = got[p]
        print(p, "max |tensor - model| %.3e, max |mean - model| %.3e, sum error %.3e of bound %.3e"
              % (np.abs(T - want).max(), np.abs(mean - want_mean).max(), abs(float(s - sum_ref)), float(64 * U * abs_ref)))
    for p in PATHS:
        T, mean, s, s2 = got[p]
        assert _same_bits(T, got["host"][0]), "%s: the tensor differs from the unfused host path" % p
        assert _same_bits(mean, got["host"][1]), "%s: the rest shape differs from the unfused host path" % p
        assert _same_bits(T, want), "%s: the tensor differs from the model" % p
        assert _same_bits(mean, want_mean), "%s: the rest shape differs from the model" % p
        assert abs(s - sum_ref) <= 64 * U * abs_ref, (p, s, sum_ref)
        if s2 is not None:
            assert abs(s2 - sq_ref) <= 64 * U * sq_ref, (p, s2, sq_ref)
    # the fused calls report sum(x^2) exactly where one sweep computes it: rest shape "first"
    assert (got["host_fused"][3] is not None) == (code == 0) and (got["device_fused"][3] is not None) == (code == 0)


@pytest.mark.parametrize("path", ("host_fused", "device_fused"))
def test_fused_calls_refuse_an_unknown_rest_shape_and_the_engine_stays_usable(path):
    import torch
    from animsnapbases_amd import HipEngine
    X, massL = _inputs(5)
    v0, n_loc = 2, 3
    e = HipEngine(0)
    try:
        shard = torch.from_numpy(np.ascontiguousarray(X[:, v0:v0 + n_loc])).to("cuda:0")
        torch.cuda.synchronize()
        sums = np.zeros(2)
        if path == "host_fused":
            rc = e.lib.asb_snapshots_upload_rest(e.h, _lib.ptr(X), 5, N, v0, n_loc, _lib.ptr(massL), 2, 1, _lib.ptr(sums))
        else:
            m_loc = np.ascontiguousarray(massL[v0:v0 + n_loc])
            rc = e.lib.asb_snapshots_adopt_dev_rest(e.h, shard.data_ptr(), 5, n_loc, _lib.ptr(m_loc), v0, N, 2, 1, _lib.ptr(sums))
        assert rc == -1, rc                                   # ASB_ERR_ARG
        assert b"rest shape" in e.lib.asb_last_error(e.h)
        with pytest.raises(RuntimeError, match="status -1"):
            if path == "host_fused":
                e.upload_rest(X, v0, n_loc, massL, 2, True)
            else:
                e.adopt_device_rest(shard.data_ptr(), 5, n_loc, massL[v0:v0 + n_loc], v0, N, 2, True)
        want, want_mean = _model(X, massL, v0, n_loc, 0, True)
        if path == "host_fused":
            e.upload_rest(X, v0, n_loc, massL, 0, True)
        else:
            e.adopt_device_rest(shard.data_ptr(), 5, n_loc, massL[v0:v0 + n_loc], v0, N, 0, True)
        assert _same_bits(e.download_snapshots(), want)
        assert _same_bits(e.get_mean(), want_mean)
    finally:
        e.close()
