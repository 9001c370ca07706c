"""The accumulation by runs (csrc/msm_kernels.hpp k_runs_hist / k_runs_scatter / k_accum_runs): one whole bucket run per thread, the
buckets in order of their run length, chosen on the device against the chunked accumulation (k_accum_l0 + k_segscan) by a flag the
table kernels raise when a run is longer than the cap.  Everything runs with accum_runs = 2 (wherever the LDS sort runs) at the bottom of
the bucket pipeline's range -- c = 12 (17 + 4 windows) up to 18 999 pairs, c = 13 (10 + 9) above -- and three ways: the cap huge (the
new kernel surely runs), the cap 1 (the chunked accumulation runs wherever a run has two entries), and accum_runs = 0.  All three give
the C oracle's 64 bytes."""
import ctypes
import random

import pytest

from helpers import Q
from oracle import cbind
from oracle.ec import INF

pytestmark = pytest.mark.gpu

HUGE = 1 << 30
NPTS = 20000


@pytest.fixture(scope="module")
def gp():
    import gpu_common
    return gpu_common


@pytest.fixture(scope="module")
def pool(gp):
    """NPTS distinct points, built once."""
    pts, _ = gp.rand_points(NPTS, 4242)
    return pts


@pytest.fixture()
def eng(gp):
    e = gp.engine()
    yield e
    for k, v in (("accum_runs", 1), ("accum_runs_cap", 0), ("async_lanes", 0), ("graphs", 0), ("slice_n", 0), ("slice_min", 0)):
        e.set_option(k, v)


WAYS = [("runs", 2, HUGE), ("chunks", 2, 1), ("off", 0, 0)]


def three_ways(eng, call, want, what, lanes=(0,)):
    """Every way gives `want`, and the device's flag (bpmi_debug_msm_runs) says the way ran that was meant: with the cap out of reach
    k_accum_runs, with cap 1 the chunked accumulation as soon as some run has two entries, with the option off nothing is planned."""
    for name, runs, cap in WAYS:
        eng.set_option("accum_runs", runs)
        eng.set_option("accum_runs_cap", cap)
        assert call() == want, (what, name)
        for lane in lanes:
            st = eng.msm_runs_state(lane)
            assert st["planned"] == (runs != 0), (what, name, lane, st)
            if name == "runs":
                assert not st["long_run"], (what, name, lane, st)
            if name == "off":
                assert not st["long_run"] and st["runs"] == 0, (what, name, lane, st)
    return st


def run_lengths(es, n):
    """{(window, |digit|): entries} of the signed-digit recoding the pipeline uses at n pairs (csrc/msm_kernels.hpp for_each_digit, mixed
    window widths: c = 12 as 17 + 4 windows below 19 000 pairs, c = 13 as 10 + 9 from there)."""
    c = 12 if n < 19000 else 13
    W = 256 // c
    wide = 256 - W * c
    runs = {}
    for e in es:
        s = e % Q
        if s > (Q - 1) // 2:
            s = Q - s
        carry = 0
        for w in range(W):
            wd = c + (1 if w + wide >= W else 0)
            t = (s & ((1 << wd) - 1)) + carry
            s >>= wd
            if t > (1 << (wd - 1)):
                b, carry = (1 << wd) - t, 1
            else:
                b, carry = t, 0
            if b:
                runs[(w, b)] = runs.get((w, b), 0) + 1
    return runs


def shape(name, pool):
    """-> (points, scalars as integers that may be unreduced)"""
    rnd = random.Random("runs/" + name)
    if name == "uniform_c12":
        n = 8449
        return pool[:n], [rnd.randrange(Q) for _ in range(n)]
    if name == "uniform_c13":
        n = 19001
        return pool[:n], [rnd.randrange(Q) for _ in range(n)]
    if name == "all_equal":                  # one run of n entries per window, in one thread
        n = 9000
        return pool[:n], [rnd.randrange(Q)] * n
    if name == "zero_one_minus_one":
        n = 10000
        return pool[:n], [rnd.choice((0, 1, Q - 1)) for _ in range(n)]
    if name == "all_zero":                   # no entry at all: nruns = 0
        n = 8500
        return pool[:n], [0] * n
    if name == "one_nonzero":
        n = 8500
        return pool[:n], [0] * 5000 + [rnd.randrange(Q)] + [0] * (n - 5001)
    if name == "range_proof_bits":           # bits, bits - 1, one blinding factor every 4 096 entries
        n = 16385
        return pool[:n], [rnd.randrange(Q) if i % 4096 == 0 else (rnd.randrange(2) if i < n // 2 else (rnd.randrange(2) - 1) % Q) for i in range(n)]
    if name == "unreduced_and_half_order":
        n = 9001
        half = (Q - 1) // 2
        edge = [Q, Q + 1, (1 << 256) - 1, 1 << 255, half, half + 1, half - 1, Q - 1, Q - 2, 2, ((1 << 255) - 1) % Q]
        return pool[:n], [edge[rnd.randrange(len(edge))] if i % 3 == 0 else rnd.randrange(Q) for i in range(n)]
    if name == "identity_points":
        n = 9000
        return [INF if i % 3 == 0 else p for i, p in enumerate(pool[:n])], [rnd.randrange(Q) for _ in range(n)]
    if name == "same_point_twice":           # P, P with one scalar: the two meet in every bucket of theirs (doubling)
        n = 9000
        es = [rnd.randrange(Q) for _ in range(n // 2)]
        return [p for p in pool[: n // 2] for _ in (0, 1)], [e for e in es for _ in (0, 1)]
    if name == "cancel_then_more":           # P, -P, R, T with one scalar: the accumulator returns to the identity and the run goes on
        n = 9000
        es = [rnd.randrange(Q) for _ in range(n // 4)]
        pts = []
        for i in range(n // 4):
            pts += [pool[i], -pool[i], pool[n // 4 + 2 * i], pool[n // 4 + 2 * i + 1]]
        return pts, [e for e in es for _ in range(4)]
    raise KeyError(name)


SHAPES = ["uniform_c12", "uniform_c13", "all_equal", "zero_one_minus_one", "all_zero", "one_nonzero", "range_proof_bits",
          "unreduced_and_half_order", "identity_points", "same_point_twice", "cancel_then_more"]
_packed = {}


def packed(name, pool):
    """-> (point bytes, scalar bytes, n, the oracle's result), computed once per shape"""
    if name not in _packed:
        pts, es = shape(name, pool)
        pb, sb = cbind.pack_points(pts), b"".join(e.to_bytes(32, "little") for e in es)
        _packed[name] = (pb, sb, len(es), cbind.msm_bytes(pb, sb, len(es)))
    return _packed[name]


@pytest.mark.parametrize("name", SHAPES)
def test_runs_chunks_and_off_give_the_oracle_result(eng, pool, name):
    pb, sb, n, want = packed(name, pool)
    assert eng.msm_geometry(n)["kernel"] == "pipeline" and eng.msm_geometry(n)["window_bits"] == (12 if n < 19000 else 13)
    three_ways(eng, lambda: eng.msm_bytes(pb, sb, n), want, name)
    # the device's own count of the runs and its flag against the recoding done here
    runs = run_lengths(shape(name, pool)[1], n)
    for cap in (HUGE, 1):
        eng.set_option("accum_runs", 2)
        eng.set_option("accum_runs_cap", cap)
        assert eng.msm_bytes(pb, sb, n) == want
        st = eng.msm_runs_state()
        up = cap == 1 and max(runs.values(), default=0) > 1
        assert st == {"planned": True, "long_run": up, "runs": 0 if up else len(runs)}, (name, cap, st, len(runs))


@pytest.mark.parametrize("name", ["uniform_c12", "uniform_c13"])
def test_uniform_run_counts_fill_no_whole_wave_or_block(pool, name):
    """What the uniform shapes are chosen for: the last wave and the last block of k_accum_runs are partly idle."""
    _, es = shape(name, pool)
    nruns = len(run_lengths(es, len(es)))
    assert nruns % 64 != 0 and nruns % 256 != 0 and nruns > 256


def test_three_segments(eng, pool):
    ns = [3000, 5000, 1500]
    rnd = random.Random(77)
    bufs, allp, alls, at = [], b"", b"", 0
    for m in ns:
        pb = cbind.pack_points(pool[at: at + m])
        sb = cbind.pack_scalars([rnd.randrange(Q) for _ in range(m)])
        bufs.append((eng.upload(pb), eng.upload(sb)))
        allp += pb
        alls += sb
        at += m
    want = cbind.msm_bytes(allp, alls, sum(ns))
    P = (ctypes.c_void_p * 3)(*[b[0].ptr for b in bufs])
    S = (ctypes.c_void_p * 3)(*[b[1].ptr for b in bufs])
    N = (ctypes.c_uint64 * 3)(*ns)

    def call():
        out = ctypes.create_string_buffer(64)
        assert eng.lib.bpmi_msm_segs_dev(eng.ctx, 3, P, S, N, out) == 0
        return out.raw
    try:
        three_ways(eng, call, want, "segments")
    finally:
        for b in bufs:
            b[0].free()
            b[1].free()


def test_cap_at_the_longest_run_and_one_below(eng, pool):
    """Uniform scalars and 40 copies of one: the longest run has exactly L entries (counted here with the pipeline's recoding).  cap = L:
    no run is longer, k_accum_runs adds it; cap = L - 1: the flag is up and the chunked accumulation does."""
    n = 9000
    rnd = random.Random(5)
    es = [rnd.randrange(Q) for _ in range(n - 40)] + [rnd.randrange(Q)] * 40
    longest = max(run_lengths(es, n).values())
    assert 40 <= longest < 72                  # (72: the rule's cap at this size)
    pb, sb = cbind.pack_points(pool[:n]), cbind.pack_scalars(es)
    want = cbind.msm_bytes(pb, sb, n)
    eng.set_option("accum_runs", 2)
    nruns = len(run_lengths(es, n))
    for cap in (longest, longest - 1, longest + 1):
        eng.set_option("accum_runs_cap", cap)
        assert eng.msm_bytes(pb, sb, n) == want, (longest, cap)
        up = cap < longest                       # the flag goes up for a run LONGER than the cap, not for one that reaches it
        assert eng.msm_runs_state() == {"planned": True, "long_run": up, "runs": 0 if up else nruns}, (longest, cap)


def test_two_lanes_flag_is_reset_for_every_msm(eng, pool):
    """Slots 0 and 1 alternating on two lanes, six MSMs, the cap by the rule: uniform scalars stay under it, equal scalars and the
    range-proof bits pass it -- every lane sees the flag down, up and down again."""
    order = ["uniform_c12", "uniform_c13", "all_equal", "range_proof_bits", "uniform_c13", "uniform_c12"]
    data = {name: packed(name, pool) for name in set(order)}
    dev = {name: (eng.upload(d[0]), eng.upload(d[1])) for name, d in data.items()}
    try:
        eng.set_option("accum_runs", 2)
        eng.set_option("accum_runs_cap", 0)
        eng.set_option("async_lanes", 1)
        eng.msm_dev_enqueue(0, dev[order[0]][0], dev[order[0]][1], data[order[0]][2])
        for j, name in enumerate(order):
            if j + 1 < len(order):
                nxt = order[j + 1]
                eng.msm_dev_enqueue((j + 1) & 1, dev[nxt][0], dev[nxt][1], data[nxt][2])
            assert eng.msm_finish(j & 1) == data[name][3], (j, name)
            st = eng.msm_runs_state(j & 1)       # (waits for the lane: the pipeline drains here, the results above are what is checked)
            assert st["planned"] and st["long_run"] == (name in ("all_equal", "range_proof_bits")), (j, name, st)
    finally:
        eng.set_option("async_lanes", 0)
        for d in dev.values():
            d[0].free()
            d[1].free()


def test_sliced_with_a_small_slice(eng, pool):
    """slice_n = 2^16: 140 001 pairs as three slices of 46 667 pairs (c = 13), two in flight; points tiled from D distinct ones, so
    the oracle's MSM is over D pairs with the column sums of the scalars."""
    n, D = 140001, 1 << 10
    rnd = random.Random(140001)
    es = [rnd.randrange(Q) for _ in range(n)]
    folded = [0] * D
    for i, e in enumerate(es):
        folded[i % D] = (folded[i % D] + e) % Q
    small = cbind.pack_points(pool[:D])
    want = cbind.msm_bytes(small, cbind.pack_scalars(folded), D)
    pb, sb = (small * (n // D + 1))[: 64 * n], cbind.pack_scalars(es)
    eng.set_option("slice_n", 1 << 16)
    assert eng.msm_geometry(n)["slices"] == 3
    three_ways(eng, lambda: eng.msm_bytes(pb, sb, n), want, "sliced")


def test_graph_replayed_twice(eng, pool):
    pb, sb, n, want = packed("uniform_c12", pool)
    d_p, d_s = eng.upload(pb), eng.upload(sb)
    try:
        eng.set_option("graphs", 1)
        for name, runs, cap in WAYS:
            eng.set_option("accum_runs", runs)
            eng.set_option("accum_runs_cap", cap)
            for k in range(3):                 # captured, replayed, replayed
                assert eng.msm_dev(d_p, d_s, n) == want, (name, k)
    finally:
        eng.set_option("graphs", 0)
        d_p.free()
        d_s.free()


def test_defaults_at_2e19(gp, eng, pool):
    """The one case at a real size: 2^19 pairs with the default options (the accumulation by runs is on from here, c = 16), synchronous and
    with equal scalars (the device falls back).  Points tiled from D distinct ones."""
    import numpy as np
    n, D = 1 << 19, 1 << 11
    small = cbind.pack_points(pool[:D])
    rng = np.random.default_rng(19)
    e = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    e[:, 7] &= 0x7FFFFFFF
    col = e.reshape(n // D, D, 8).astype(np.uint64).sum(axis=0)
    folded = []
    for j in range(D):
        v = 0
        for k in range(7, -1, -1):
            v = (v << 32) + int(col[j, k])
        folded.append(v % Q)
    want = cbind.msm_bytes(small, cbind.pack_scalars(folded), D)
    d_p, d_s = eng.upload(small * (n // D)), eng.upload(e.tobytes())
    one = rng.integers(1, 1 << 62)
    d_one = eng.upload(int(one).to_bytes(32, "little") * n)
    want_one = cbind.msm_bytes(small, cbind.pack_scalars([int(one) * (n // D) % Q] * D), D)
    try:
        assert eng.msm_geometry(n)["window_bits"] == 16
        assert eng.msm_dev(d_p, d_s, n) == want
        st = eng.msm_runs_state()
        assert st["planned"] and not st["long_run"] and (1 << 18) < st["runs"] <= (1 << 19), st       # 16 entries per bucket: hardly one is empty
        assert eng.msm_dev(d_p, d_one, n) == want_one
        assert eng.msm_runs_state() == {"planned": True, "long_run": True, "runs": 0}
        assert eng.msm_dev(d_p, d_s, n) == want
        assert eng.msm_runs_state() == st
    finally:
        for d in (d_p, d_s, d_one):
            d.free()
