"""CPU: the host side of S^T on several ranks (constraints.st_shard_plan): every vertex has one owner, the remapped rows
of S^T over a shard and its halo give the global rows' products term by term in the global order, and the halo rows land
where the all-gather of every rank's send rows puts them."""
import numpy as np
import pytest
from scipy import sparse

from animsnapbases_amd.constraints import st_shard_plan
from animsnapbases_amd.distributed import partition


def _st(nv, ncols, seed, empty=()):
    rng = np.random.default_rng(seed)
    A = sparse.random(nv, ncols, density=6.0 / ncols, random_state=seed, format="csr")
    A.data[:] = rng.uniform(0.5, 1.5, size=A.data.shape)
    A = A.tolil()
    for v in empty:
        A[v, :] = 0
    return A.tocsr()


@pytest.mark.parametrize("world", [1, 2, 3, 5])
@pytest.mark.parametrize("seed", [0, 1])
def test_plan_reproduces_the_global_rows(world, seed):
    nv, ncols = 300, 701
    St = _st(nv, ncols, seed, empty=(0, 17, 299))
    St.eliminate_zeros()
    shards = partition(ncols, world)
    R = np.random.default_rng(seed + 9).normal(size=(ncols, 4))
    owners = np.zeros(nv, dtype=np.int64)
    plans = [st_shard_plan(St, shards, r) for r in range(world)]
    stride = plans[0]["stride"]
    gathered = np.zeros((world * stride, 4))
    for r, pl in enumerate(plans):
        v0, n = shards[r]
        assert np.all((pl["send"] >= v0) & (pl["send"] < v0 + n))
        gathered[r * stride:r * stride + len(pl["send"])] = R[pl["send"]]
    for r, pl in enumerate(plans):
        v0, n = shards[r]
        owners[pl["owned"]] += 1
        assert pl["halo_sizes"] == [len(q["halo"]) for q in plans]
        assert np.all(np.diff(pl["halo"]) > 0) and not np.any((pl["halo"] >= v0) & (pl["halo"] < v0 + n))
        H = gathered[pl["slot"]]
        assert np.array_equal(H, R[pl["halo"]])
        M = np.concatenate([R[v0:v0 + n], H])
        for i, v in enumerate(pl["owned"]):
            a, b = pl["indptr"][i], pl["indptr"][i + 1]
            ga, gb = St.indptr[v], St.indptr[v + 1]
            assert np.array_equal(pl["data"][a:b], St.data[ga:gb])
            assert np.array_equal(M[pl["slots"][a:b]], R[St.indices[ga:gb]])            # same terms, same order
            if gb > ga:
                assert v0 <= St.indices[ga] < v0 + n                                    # owner: smallest column
            else:
                assert r == 0
    assert np.all(owners == 1)
