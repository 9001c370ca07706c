"""The first two entries of a bucket run in front of k_accum_runs' loop (csrc/msm_kernels.hpp: entry 1 makes the accumulator the affine
point, entry 2 is the affine + affine addition xyzz_mmadd) and the kernel's two instantiations (dense point fetch for one array, the
segment walk otherwise).  accum_runs = 2 runs the kernel at the bottom of the bucket pipeline's range (c = 12 below 19 000 pairs, c = 13
from there).  The order of the entries inside a run is not reproducible, so every shape puts its special entries into several hundred
buckets of window 0: the other scalars keep the lower half of that window's digits, the special ones take a digit each from the upper
half, and elsewhere they spread over all buckets.  Every case is compared with the C oracle's 64 bytes, with the cap huge (the run table
takes the MSM) and with cap 1 (the chunked accumulation), as ONE dense array and split into three segments; the half-block selection
reaches the kernel through the inner-product argument's deferred round."""
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
    pts, _ = gp.rand_points(NPTS, 777)
    return pts


@pytest.fixture()
def eng(gp):
    e = gp.engine()
    for k, v in (("async_lanes", 0), ("graphs", 0)):
        e.set_option(k, v)
    yield e
    for k, v in (("accum_runs", 1), ("accum_runs_cap", 0), ("async_lanes", 0), ("graphs", 0), ("ipa_big_m", 0), ("ipa_small_m", 0)):
        e.set_option(k, v)


def windows(n):
    """[(bit offset, width)] of the pipeline's windows at n pairs: c = 12 as 17 + 4 windows below 19 000 pairs, c = 13 as 10 + 9 from there
    (the last `wide` windows are one bit wider)"""
    c = 12 if n < 19000 else 13
    W = 256 // c
    wide = 256 - W * c
    out, at = [], 0
    for w in range(W):
        wd = c + (1 if w + wide >= W else 0)
        out.append((at, wd))
        at += wd
    return out


def run_lengths(es, n):
    """{(window, |digit|): entries} of the signed-digit recoding (csrc/msm_kernels.hpp for_each_digit)"""
    runs = {}
    for e in es:
        s = e % Q
        if s > (Q - 1) // 2:
            s = Q - s
        carry = 0
        for w, (at, wd) in enumerate(windows(n)):
            t = ((s >> at) & ((1 << wd) - 1)) + carry
            if t > (1 << (wd - 1)):
                b, carry = (1 << wd) - t, 1
            else:
                b, carry = t, 0
            if b:
                runs[(w, b)] = runs.get((w, b), 0) + 1
    return runs


def scalar(rnd, n, d0=None, positive=False):
    """A scalar below 2^254 (so it is not negated by the recoding).  Digit of window 0: d0, or one of the lower half of the positive
    digits.  positive: every other window's digit positive too (its value in [1, 2^(wd - 1)], no carry), else uniform bits."""
    ws = windows(n)
    half0 = 1 << (ws[0][1] - 2)                        # window 0's positive digits are 1 .. 2 half0: background 1 .. half0, special above
    s = d0 if d0 is not None else rnd.randrange(1, half0 + 1)
    for k, (at, wd) in enumerate(ws[1:], 1):
        top = k == len(ws) - 1
        if positive:
            v = rnd.randrange(1, (1 << (wd - (3 if top else 1))) + 1)
        else:
            v = rnd.randrange(1 << (wd - (2 if top else 0)))
        s |= v << at
    assert s < 1 << 254
    return s


def shape(name, pool):
    """-> (points, scalars, {window-0 digit: entries} of the special buckets)"""
    rnd = random.Random("peel/" + name)
    n = {"sizes": 8449, "doubling": 9001, "cancel": 9500, "identity": 10007, "negative": 8777, "sizes_c13": 19501}[name]
    positive = name == "negative"
    half0 = 1 << (windows(n)[0][1] - 2)
    pts, es, special = [], [], {}
    fresh = iter(pool)                                  # every pair its own point, unless the pattern says otherwise
    groups = 900 if n < 19000 else 1500
    for k in range(groups):
        d = half0 + 1 + k                              # one bucket of window 0 per group
        assert d < 2 * half0
        sc = lambda: scalar(rnd, n, d, positive)
        if name in ("sizes", "negative", "sizes_c13"):  # buckets of exactly 1, 2 and 3 entries
            m = 1 + k % 3
            grp = [(next(fresh), sc()) for _ in range(m)]
        elif name == "doubling":                        # the same point twice: alone, and with a third entry
            p = next(fresh)
            grp = [(p, sc()), (p, sc())] + ([(next(fresh), sc())] if k % 2 else [])
        elif name == "cancel":                          # s and q - s of one point: the identity after two entries; alone, and with a third entry
            p, s = next(fresh), sc()
            grp = [(p, s), (p, Q - s)] + ([(next(fresh), sc())] if k % 2 else [])
        else:                                           # identity points: the only entry, one of two, two of three
            grp = [[(INF, sc())], [(INF, sc()), (next(fresh), sc())], [(INF, sc()), (INF, sc()), (next(fresh), sc())]][k % 3]
        special[d] = len(grp)
        pts += [g[0] for g in grp]
        es += [g[1] for g in grp]
    while len(es) < n:
        pts.append(next(fresh))
        es.append(scalar(rnd, n, None, positive))
    order = list(range(n))
    rnd.shuffle(order)
    pts, es = [pts[i] for i in order], [es[i] for i in order]
    if name == "negative":                              # q - s: the recoding negates the scalar, every digit of every entry is negative
        es = [Q - e for e in es]
    return pts, es, special


SHAPES = ["sizes", "doubling", "cancel", "identity", "negative", "sizes_c13"]
_packed = {}


def packed(name, pool):
    if name not in _packed:
        pts, es, special = shape(name, pool)
        pb, sb = cbind.pack_points(pts), b"".join(e.to_bytes(32, "little") for e in es)
        _packed[name] = (pb, sb, len(es), cbind.msm_bytes(pb, sb, len(es)), run_lengths(es, len(es)), special)
    return _packed[name]


def both_caps(eng, call, want, runs, what, lanes=(0,)):
    """cap huge: the run table takes the MSM (k_accum_runs); cap 1: the chunked accumulation, as soon as a run has two entries"""
    for cap in (HUGE, 1):
        eng.set_option("accum_runs", 2)
        eng.set_option("accum_runs_cap", cap)
        assert call() == want, (what, cap)
        for lane in lanes:
            st = eng.msm_runs_state(lane)
            assert st["planned"], (what, cap, st)
            if cap == HUGE:
                assert not st["long_run"], (what, st)
                if runs is not None:
                    assert st["runs"] == len(runs), (what, st, len(runs))
            elif runs is not None:
                assert st["long_run"] == (max(runs.values()) > 1), (what, st)


@pytest.mark.parametrize("name", SHAPES)
def test_shape_is_what_it_says(pool, name):
    """Host only: the special buckets hold exactly their entries, and the table's last wave is not full."""
    _, _, n, _, runs, special = packed(name, pool)
    assert 8449 <= n <= 20000 and len(special) >= 300
    for d, m in special.items():
        assert runs[(0, d)] == m, (name, d)
    assert {1, 2, 3} & set(special.values()) and len(runs) % 64 != 0 and len(runs) > 256
    if name == "negative":
        assert all(e > (Q - 1) // 2 for e in shape(name, pool)[1])


@pytest.mark.parametrize("name", SHAPES)
def test_one_dense_array(eng, pool, name):
    pb, sb, n, want, runs, _ = packed(name, pool)
    assert eng.msm_geometry(n)["kernel"] == "pipeline" and eng.msm_geometry(n)["window_bits"] == (12 if n < 19000 else 13)
    both_caps(eng, lambda: eng.msm_bytes(pb, sb, n), want, runs, name)


@pytest.mark.parametrize("name", SHAPES)
def test_three_segments(eng, pool, name):
    pb, sb, n, want, runs, _ = packed(name, pool)
    ns = [n // 3 + 1, n // 2 - 7]
    ns.append(n - sum(ns))
    bufs, at = [], 0
    for m in ns:
        bufs.append((eng.upload(pb[64 * at: 64 * (at + m)]), eng.upload(sb[32 * at: 32 * (at + m)])))
        at += m
    P = (ctypes.c_void_p * 3)(*[b[0].ptr for b in bufs])
    S = (ctypes.c_void_p * 3)(*[b[1].ptr for b in bufs])
    N = (ctypes.c_uint64 * 3)(*ns)

    def call():
        out = ctypes.create_string_buffer(64)
        assert eng.lib.bpmi_msm_segs_dev(eng.ctx, 3, P, S, N, out) == 0
        return out.raw
    try:
        both_caps(eng, call, want, runs, name + " in three segments")
    finally:
        for b in bufs:
            b[0].free()
            b[1].free()


def test_half_block_selection(eng, pool):
    """The inner-product argument over 16 384 generators: round 1 is a three-segment MSM of 16 385 pairs, and after a deferred fold round 2
    is the MSM over the UNFOLDED generators through the half-block selection (blocks of 8 192, one half each).  With the challenge 1 the
    folded vectors are a_lo + a_hi and b_lo + b_hi whatever the convention, and the two generators that fold into one carry the same
    scalar: they meet in every bucket.  Several hundred such pairs are one point twice (the doubling of the second entry), several hundred
    a point and its negative (the identity after two entries), alone in their bucket of window 0 or with a second pair."""
    n, half, quarter = 1 << 14, 1 << 13, 1 << 12
    rnd = random.Random("peel/half-block")
    g, h = list(pool[:n]), list(reversed(pool[1:n + 1]))
    u = pool[0]
    half0 = 1 << (windows(n + 1)[0][1] - 2)
    av = [scalar(rnd, n + 1) for _ in range(half)]      # a_lo (a_hi = 0): the folded a
    bv = [scalar(rnd, n + 1) for _ in range(half)]      # b_lo (b_hi = 0): the folded b
    for j in range(900):
        d = half0 + 1 + j
        for lo in (0, quarter):                         # L uses a'[:quarter] with g's upper halves, R a'[quarter:] with the lower ones
            av[lo + j] = scalar(rnd, n + 1, d)
            gi = (quarter - lo) + j                     # the generator pair g[gi], g[gi + half] of that scalar
            if j < 300:
                g[gi + half] = g[gi]
            elif j < 600:
                g[gi + half] = -g[gi]
            else:                                       # a pair of h that cancels, beside the two distinct generators of g
                bv[(quarter - lo) + j] = scalar(rnd, n + 1, d)
                h[lo + j + half] = -h[lo + j]
    a, b = av + [0] * half, bv + [0] * half
    eng.set_option("ipa_big_m", 1 << 10)
    eng.set_option("ipa_small_m", 1)
    # round 2 as explicit pairs
    La, Lb = av[:quarter], bv[quarter:]
    Ra, Rb = av[quarter:], bv[:quarter]
    wantL = cbind.msm(g[quarter:half] + g[half + quarter:] + h[:quarter] + h[half:half + quarter] + [u], La + La + Lb + Lb + [cbind.sc_dot(La, Lb)])
    wantR = cbind.msm(g[:quarter] + g[half:half + quarter] + h[quarter:half] + h[half + quarter:] + [u], Ra + Ra + Rb + Rb + [cbind.sc_dot(Ra, Rb)])
    want1L = cbind.msm(g[half:] + [u], av + [0])        # round 1: c_L = <a_lo, b_hi> = 0
    want1R = cbind.msm(h[half:] + [u], bv + [0])
    for cap in (HUGE, 1):
        eng.set_option("accum_runs", 2)
        eng.set_option("accum_runs_cap", cap)
        st = eng.ipa_create(cbind.pack_points(g), cbind.pack_points(h), cbind.pack_scalars(a), cbind.pack_scalars(b), n, cbind.pack_points([u]))
        try:
            L, R = st.round_LR()
            assert (L, R) == (cbind.pack_points([want1L]), cbind.pack_points([want1R])), cap
            st.fold(1, 1)
            assert len(st) == half
            L, R = st.round_LR()
            assert (L, R) == (cbind.pack_points([wantL]), cbind.pack_points([wantR])), cap
            for lane in (0, 1):
                s = eng.msm_runs_state(lane)
                assert s["planned"] and s["long_run"] == (cap == 1), (cap, lane, s)
        finally:
            st.close()
