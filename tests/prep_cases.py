"""The case table and the data families of the snapshot-preparation tests (test_prep_model_cpu.py, test_gpu_prep.py).

A row is (F, n_loc, shard, mass, code, subtract, family).  The table is not a full product: every F of F_VALUES meets both rest
shapes with and without massL (four rows), the n_loc values and the shard form go round underneath, and four rows carry the
large shard.  EDGES names what each value is there for; test_prep_model_cpu.py asserts that every edge occurs in some row with
both rest shapes and with and without massL.
"""
import collections

import numpy as np

from prep_model import pad16

Row = collections.namedtuple("Row", "F n_loc N v0 mass code subtract family")

F_VALUES = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 145, 1000)
N_VALUES = (1, 2, 10, 11, 21, 22, 43, 342)
N_LARGE = 11000
F_LARGE = (3, 17)


def _rows():
    rows = []
    for fi, F in enumerate(F_VALUES):
        for c in range(4):
            code, mass = c & 1, bool(c >> 1)
            n_loc = N_VALUES[(fi + 2 * c) % 8]
            shard = (fi + c) % 2 == 1
            rows.append(Row(F, n_loc, n_loc + 5 if shard else n_loc, 3 if shard else 0, mass, code, (fi + (c >> 1)) % 2 == 0,
                            "integer" if (fi + c) % 3 else "generic"))
    for i, (F, code, mass) in enumerate(((3, 0, True), (3, 1, False), (17, 0, False), (17, 1, True))):
        rows.append(Row(F, N_LARGE, N_LARGE + (4 if i & 1 else 0), 4 if i & 1 else 0, mass, code, i < 2, "integer" if i % 2 == 0 else "generic"))
    return rows


ROWS = _rows()


def row_id(r):
    return "F%d-n%d%s-%s-code%d-%s-%s" % (r.F, r.n_loc, "s" if r.N != r.n_loc else "", "m" if r.mass else "u", r.code,
                                         "sub" if r.subtract else "raw", r.family)


EDGES = collections.OrderedDict()
for _F in F_VALUES:
    EDGES["F=%d" % _F] = (lambda r, F=_F: r.F == F)
for _n in N_VALUES + (N_LARGE,):
    EDGES["n_loc=%d" % _n] = (lambda r, n=_n: r.n_loc == n)
EDGES.update({
    "second 32-frame tile of the transposes": lambda r: r.F > 32,
    "partial 32-frame tile": lambda r: r.F % 32 != 0,
    "whole 32-frame tiles only": lambda r: r.F % 32 == 0,
    "lane loop of k_center / k_sqdev (F > 64)": lambda r: r.F > 64,
    "exactly the 64 lanes": lambda r: r.F == 64,
    "double2 lane loop of k_scale_energy (Fp / 2 > 64)": lambda r: pad16(r.F) // 2 > 64,
    "pad width 0": lambda r: pad16(r.F) - r.F == 0,
    "pad width 1": lambda r: pad16(r.F) - r.F == 1,
    "pad width 14": lambda r: pad16(r.F) - r.F == 14,
    "pad width 15": lambda r: pad16(r.F) - r.F == 15,
    "one partial strip of 32 columns": lambda r: 3 * r.n_loc < 32,
    "second strip of 32 columns": lambda r: 3 * r.n_loc > 32,
    "strips: one column over (C = 33, 129)": lambda r: (3 * r.n_loc) % 32 == 1,
    "strips: one column short (C = 63)": lambda r: (3 * r.n_loc) % 32 == 31,
    "shard inside a larger N": lambda r: r.N != r.n_loc and r.v0 > 0,
    "whole range": lambda r: r.N == r.n_loc,
    "more than 1024 strips (k_sum_pairs loops)": lambda r: (3 * r.n_loc + 31) // 32 > 1024,
    "more than 1024 vertices (k_ev_moments loops)": lambda r: r.n_loc > 1024,
})


def large_grid_facts(cap):
    """what the n_loc = N_LARGE rows are there for, from the context's grid cap: asserted, not assumed"""
    rows_want, e_want = (3 * N_LARGE + 3) // 4, (N_LARGE + 3) // 4
    return {
        "row_grid is capped, several rounds, a partial last one": rows_want > 2 * cap and rows_want % cap != 0,
        "k_scale_energy's grid is capped, a partial last round": e_want > cap and e_want % cap != 0,
        "k_e0_finish sees more than 256 partials": min(e_want, cap) > 256,
        "k_sum_pairs sees more than 1024 strips": (3 * N_LARGE + 31) // 32 > 1024,
        "k_ev_moments sees more than 1024 values": N_LARGE > 1024,
    }


# ------------------------------------------------------------------------------------------------ data families
def _seed(r):
    return [r.F, r.n_loc, r.N, int(r.mass), r.code, int(r.subtract)]


def integer_data(r):
    """integer X in [-8 - F, 8], massL in {1, 2, 4}; for rest shape 1 the last frame is lowered so that every column sum is a
    multiple of F: the mean, hence every entry after the subtraction, is an integer and every sum is exact in any order"""
    rng = np.random.default_rng([1] + _seed(r))
    X = rng.integers(-8, 9, size=(r.F, r.N, 3)).astype(np.float64)
    if r.code == 1:
        X[-1] -= np.mod(X.sum(axis=0), r.F)
    massL = 2.0 ** rng.integers(0, 3, size=r.N) if r.mass else None
    return X, massL


def generic_data(r):
    """a normal animation plus a per-vertex offset, per-vertex scales from 1e-6 to 1e6"""
    rng = np.random.default_rng([2] + _seed(r))
    scale = 10.0 ** rng.uniform(-6, 6, size=(1, r.N, 1))
    X = (rng.standard_normal((r.F, r.N, 3)) + 3.0 * rng.standard_normal((1, r.N, 3))) * scale
    massL = rng.uniform(0.5, 2.0, r.N) if r.mass else None
    return X, massL


def offset_data(F, N, seed=0):
    """coordinates near 1e6 with motion of order 1: cancellation in x - mean, and in E0 - m_v without the subtraction"""
    rng = np.random.default_rng([3, F, N, seed])
    return 1e6 * (1.0 + rng.uniform(0, 1, size=(1, N, 3))) + rng.standard_normal((F, N, 3))


def still_data(F, N, moving=(), seed=0):
    """vertices constant in time, except those of `moving` (order-1 motion; the same motion on all of them)"""
    rng = np.random.default_rng([4, F, N, seed])
    X = np.repeat(rng.uniform(-3, 3, size=(1, N, 3)), F, axis=0)
    motion = rng.standard_normal((F, 1, 3))
    motion -= motion.mean(axis=0, keepdims=True)
    for v in moving:
        X[:, v] = motion[:, 0]
    return X


def translated_data(F, N, d=100.0, sigma=1e-3, seed=0):
    """frames 1 .. F - 1 are frame 0 moved by (d, d, d), plus noise sigma << d: with rest shape "first" the standardised
    tensor has mu^2 / var = F - 1 up to sigma^2 / d^2"""
    rng = np.random.default_rng([5, F, N, seed])
    X = np.repeat(rng.uniform(-1, 1, size=(1, N, 3)), F, axis=0)
    X[1:] += d + sigma * rng.standard_normal((F - 1, N, 3))
    return X


TRANSLATED_F = {6: "one sweep", 9: "one sweep", 13: "second pass", 17: "second pass"}


def data(r):
    return integer_data(r) if r.family == "integer" else generic_data(r)
