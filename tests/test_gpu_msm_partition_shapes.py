"""Level A of the LDS sort (csrc/msm_kernels.hpp k_partition): a thread reads eight codes per 16-byte load from the first aligned code of
its window, the codes before it and behind the last whole vector one by one.  Sizes at the bottom of the LDS sort's range (tiles of 4 096 scalars) and around 2^19 (tiles of 16 384), whose window bases are
aligned (n = 0 mod 8) or not (head and tail run), scalar shapes that fill one partition, none, or the two ends of every tile.  Everything
with accum_runs = 2 (the accumulation by runs behind the sort at every size); every case gives the C oracle's 64 bytes.
Points are tiled from D distinct ones, so the oracle's MSM is over D pairs with the column sums of the scalars."""
import numpy as np
import pytest

from helpers import Q
from oracle import cbind

pytestmark = pytest.mark.gpu

D = 1 << 11
SIZES = [8449, 12287, 12289, 16384, 1 << 19, (1 << 19) + 1, (1 << 19) + 16383]
SHAPES = ["uniform", "all_equal", "zero_one_minus_one", "all_zero", "tile_ends"]
NMAX = max(SIZES)


@pytest.fixture(scope="module")
def gp():
    import gpu_common
    return gpu_common


@pytest.fixture(scope="module")
def eng(gp):
    e = gp.engine()
    yield e
    for k, v in (("accum_runs", 1), ("async_lanes", 0)):
        e.set_option(k, v)


@pytest.fixture(scope="module")
def points(gp, eng):
    """(the D distinct points' bytes, the device array of NMAX points: point i = distinct point i mod D)"""
    pts, _ = gp.rand_points(D, 7117)
    small = cbind.pack_points(pts)
    d_p = eng.upload((small * (NMAX // D + 1))[: 64 * NMAX])
    yield small, d_p
    d_p.free()


def scalars(name, n):
    """-> n x 8 uint32 words (little-endian scalars below q)"""
    rng = np.random.default_rng([n, SHAPES.index(name)])
    e = np.zeros((n, 8), dtype=np.uint32)

    def uniform(m):
        u = rng.integers(0, 1 << 32, size=(m, 8), dtype=np.uint64).astype(np.uint32)
        u[:, 7] &= 0x7FFFFFFF                      # below 2^255 < q
        return u
    if name == "uniform":
        e = uniform(n)
    elif name == "all_equal":                      # one partition takes a whole window (the heavy path from 2^19 pairs)
        e[:] = uniform(1)
    elif name == "zero_one_minus_one":
        vals = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in (0, 1, Q - 1)), dtype=np.uint32).reshape(3, 8)
        e = vals[rng.integers(0, 3, size=n)]
    elif name == "all_zero":                       # every code DIG_NONE
        pass
    elif name == "tile_ends":                      # the first and the last scalar of every tile, of the last (partial) one too
        ts = 16384 if n >= (1 << 19) else 4096
        idx = sorted(set(list(range(0, n, ts)) + list(range(ts - 1, n, ts)) + [n - 1]))
        e[idx] = uniform(len(idx))
    else:
        raise KeyError(name)
    return np.ascontiguousarray(e)


def oracle(small, e):
    """the MSM of scalars e over the tiled points: D pairs with the column sums"""
    n = e.shape[0]
    rows = -(-n // D)
    pad = np.zeros((rows * D, 8), dtype=np.uint64)
    pad[:n] = e
    col = pad.reshape(rows, D, 8).sum(axis=0)
    folded = []
    for j in range(D):
        v = 0
        for k in range(7, -1, -1):
            v = (v << 32) + int(col[j, k])
        folded.append(v % Q)
    return cbind.msm_bytes(small, cbind.pack_scalars(folded), D)


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("n", SIZES)
def test_the_oracle_result(eng, points, n, name):
    small, d_p = points
    e = scalars(name, n)
    want = oracle(small, e)
    d_s = eng.upload(e.tobytes())
    try:
        eng.set_option("accum_runs", 2)
        geo = eng.msm_geometry(n)
        assert geo["kernel"] == "pipeline" and geo["window_bits"] == (12 if n < 19000 else 16), geo        # the LDS sort: c >= 10
        assert eng.msm_dev(d_p, d_s, n) == want, (n, name)
        assert eng.msm_runs_state()["planned"], (n, name)
    finally:
        eng.set_option("accum_runs", 1)
        d_s.free()


def test_two_lanes_beside_a_run_accumulation(eng, points):
    """Four MSMs of 2^19 pairs with different scalars, slots 0 and 1 alternating on two lanes with the options at their defaults: level A of
    one MSM runs beside the other's accumulation by runs."""
    small, d_p = points
    n = 1 << 19
    es = []
    for k in range(4):
        rng = np.random.default_rng(9000 + k)
        e = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
        e[:, 7] &= 0x7FFFFFFF
        es.append(e)
    wants = [oracle(small, e) for e in es]
    assert len(set(wants)) == 4
    devs = [eng.upload(e.tobytes()) for e in es]
    try:
        eng.set_option("accum_runs", 1)
        eng.set_option("async_lanes", 1)
        eng.msm_dev_enqueue(0, d_p, devs[0], n)
        for j in range(4):
            if j + 1 < 4:
                eng.msm_dev_enqueue((j + 1) & 1, d_p, devs[j + 1], n)
            assert eng.msm_finish(j & 1) == wants[j], j
            st = eng.msm_runs_state(j & 1)
            assert st["planned"] and not st["long_run"], (j, st)
    finally:
        eng.set_option("async_lanes", 0)
        for d in devs:
            d.free()
