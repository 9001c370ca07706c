"""GPU parity of the fixed-base MSM (bpmi_fixed_base_*, bpmi_msm_fixed*; FixedBasePoints, vector_commitment_fixed): an object that
owns a generator list and the table T[r][i] = 2^(c Wv r) P_i of its multiples, so that the W windows of a scalar run as Wv = ceil(W / R)
virtual windows over n R virtual pairs.  Replaces Pippenger.multiexp (src/pippenger/pippenger.py:22-61) and vector_commitment
(src/utils/commitments.py:13) over generators that never change.  Every result is compared bit for bit with the C oracle's MSM of the
same points and scalars, the larger and skewed ones also with bpmi_msm_dev; every (window bits, rows) is forced, so the tests do not
depend on the measured automatic rule."""
import ctypes
import json
import os
import random
import subprocess

import pytest

import point_edge_cases as pec
from helpers import Q
from oracle import cbind
from oracle.ec import INF, Point as OP, secp256k1 as OC

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF = (Q - 1) // 2
SETTINGS = [(16, 16), (16, 4), (16, 5), (13, 20), (13, 3), (12, 2), (10, 26), (16, 1)]
SIZES = [1, 2, 63, 64, 65, 257, 1000, 4097]
SHAPES = ["uniform", "top_window_edges", "all_same", "bits01", "zeros", "above_q", "edges", "digit_edges"]


@pytest.fixture(scope="module")
def gp():
    import gpu_common
    return gpu_common


@pytest.fixture(scope="module")
def base_points(gp):
    """1 000 distinct points, repeated to the size a case needs (the oracle's cost is the scalars')."""
    return gp.rand_points(1000, 1414)[0]


def _points(base, n, shift=0):
    return [base[(i + shift) % len(base)] for i in range(n)]


def _raw(es):
    """32 bytes little-endian each, NOT reduced: the library reduces on load."""
    return b"".join(int(e).to_bytes(32, "little") for e in es)


def _digit_edge_values():
    """Scalars whose signed digits sit at the edges of a window of 16, 13 and 10 bits: a single digit of magnitude exactly 2^(w-1) in several
    positions, the same negated (q - v: the scalar's own negation beside a digit of 2^15 is what a sign folded into the code's bit 15
    breaks), 2^(w-1) in every digit, 2^(w-1) + 1 in every digit (a carry through every window) and 2^(w-1) - 1 in every digit."""
    vals = []
    for w in (16, 13, 10):
        half, nd = 1 << (w - 1), 256 // w
        for j in sorted({0, 1, 2, nd // 2, nd - 2, nd - 1}):
            v = half << (w * j)
            vals += [v % Q, (Q - v) % Q]
        for d in (half, half + 1, half - 1):
            v = sum(d << (w * j) for j in range(nd)) % Q
            vals += [v, Q - v]
    return vals


def _scalars(shape, n, rnd):
    """The shapes of tests/test_gpu_msm_batch.py, and digit_edges."""
    if shape == "uniform":
        return [rnd.randrange(Q) for _ in range(n)]
    if shape == "top_window_edges":
        vals = [HALF, HALF - 1, HALF + 1, HALF - (1 << 200), HALF + (1 << 200) + 5, (1 << 254), (1 << 254) + (1 << 253), (1 << 254) - 1,
                (1 << 240), (1 << 240) - 1, (0x4000 << 240) | 12345, (0x4001 << 240), (0x3FFF << 240) | ((1 << 240) - 1), Q - 1, Q - 2, 1, 0,
                Q - HALF, (0x7FFF << 240) % Q, ((0x7FFE << 240) | ((1 << 240) - 1)) % Q]
        return [vals[rnd.randrange(len(vals))] if i % 3 else rnd.randrange(Q) for i in range(n)]
    if shape == "all_same":
        return [rnd.randrange(Q)] * n
    if shape == "bits01":
        return [rnd.randrange(2) for _ in range(n // 2)] + [(rnd.randrange(2) - 1) % Q for _ in range(n - n // 2)]
    if shape == "zeros":
        return [0] * n
    if shape == "above_q":                     # any 256-bit value is allowed: [q, 2^256)
        return [rnd.choice((Q, Q + 1, (1 << 256) - 1, 2 * Q - 1 if 2 * Q - 1 < 1 << 256 else Q + 5, rnd.randrange(Q, 1 << 256))) for _ in range(n)]
    if shape == "edges":
        vals = [0, 1, Q - 1, HALF, HALF + 1]
        return [vals[(i + rnd.randrange(2)) % len(vals)] for i in range(n)]
    if shape == "digit_edges":
        vals = _digit_edge_values()
        off = rnd.randrange(len(vals))
        return [vals[(i + off) % len(vals)] for i in range(n)]
    raise ValueError(shape)


def _want(pts, es, m=None):
    """the oracle's MSM over the first m points and scalars (the scalars reduced mod q, as the library reduces them on load)"""
    m = len(es) if m is None else m
    return cbind.msm_bytes(cbind.pack_points(pts[:m]), cbind.pack_scalars(es[:m]), m) if m else bytes(64)


class _Fixed:
    """A fixed-base object over `pts` (uploaded; the upload is freed at once: the object copies), closed at the end of the `with`."""

    def __init__(self, eng, pts, c, rows, host=False):
        pb = cbind.pack_points(pts)
        if host:
            self.fx = eng.fixed_base_create(pb, len(pts), c, rows)
        else:
            d = eng.upload(pb)
            try:
                self.fx = eng.fixed_base_create(d, len(pts), c, rows)
            finally:
                d.free()

    def __enter__(self):
        return self.fx

    def __exit__(self, *exc):
        self.fx.close()


def _reset(eng):
    for k, v in (("accum_runs", 1), ("accum_runs_cap", 0), ("async_lanes", 0), ("validate_points", 1)):
        eng.set_option(k, v)


def _shape_of(c, rows):
    W = 255 // c + 1
    Wv = -(-W // rows)
    return W, Wv, -(-W // Wv)


# ---- the table --------------------------------------------------------------------------------------------------------------
def _table_points(base):
    """70 points: the identity (twice), G, -G, a duplicate pair, x within 256 of 0 and of p, tiny y, and random ones."""
    G = OC.G
    edge = [OP(x, y) for _, x, y in pec.small_points()[:3] + pec.near_p_points()[:3]] + [OP(x, y) for x, y in pec.tiny_y_points()[:2]]
    pts = [INF, G, OP(G.x, OC.p - G.y), base[7], base[7]] + edge + [INF]
    return pts + _points(base, 70 - len(pts), 100)


@pytest.mark.parametrize("c,rows", [(16, 16), (13, 3), (10, 26)])
def test_table_rows_are_the_multiples(gp, base_points, c, rows):
    eng = gp.engine()
    pts = _table_points(base_points)
    assert len(pts) == 70
    W, Wv, R = _shape_of(c, rows)
    finite = [i for i, p in enumerate(pts) if p != INF]
    with _Fixed(eng, pts, c, rows) as fx:
        info = fx.info
        assert (info["n"], info["window_bits"], info["windows"], info["rows"], info["virtual_windows"], info["table_bytes"]) == (70, c, W, R, Wv, 64 * 70 * R)
        for r in range(R):
            got = fx.table_bytes(r, 0, 70)
            mult = cbind.ec_mul_batch([pts[i] for i in finite], [pow(2, c * Wv * r, Q)] * len(finite))
            want = [bytes(64)] * 70                                     # the identity stays 64 zero bytes
            for i, m in zip(finite, mult):
                want[i] = cbind.pack_points([m])
            assert got == b"".join(want), (c, rows, r)
            for i in range(70):
                x, y = int.from_bytes(got[64 * i: 64 * i + 32], "little"), int.from_bytes(got[64 * i + 32: 64 * i + 64], "little")
                assert x < OC.p and y < OC.p
        assert fx.table_bytes(R - 1, 69, 1) == got[64 * 69:] and fx.table_bytes(0, 3, 2) == cbind.pack_points(pts[3:5])
        assert eng.lib.bpmi_fixed_base_table(fx.handle, R, 0, 1, ctypes.create_string_buffer(64)) == -3
        assert eng.lib.bpmi_fixed_base_table(fx.handle, 0, 69, 2, ctypes.create_string_buffer(128)) == -3


# ---- the parity grid ----------------------------------------------------------------------------------------------------------
def _grid():
    """A thinned product of the three axes: the (size, setting) pairs of one colour of the chessboard, the shape advancing along both
    axes -- every size, every setting and every shape occurs (asserted below)."""
    cases = []
    for i, n in enumerate(SIZES):
        for j, (c, rows) in enumerate(SETTINGS):
            if (i + j) % 2 == 0:
                cases.append((n, c, rows, SHAPES[((i + j) // 2 + i) % len(SHAPES)]))
    assert {x[0] for x in cases} == set(SIZES) and {x[1:3] for x in cases} == set(SETTINGS) and {x[3] for x in cases} == set(SHAPES)
    return cases


@pytest.mark.parametrize("n,c,rows,shape", _grid())
def test_parity_grid(gp, base_points, n, c, rows, shape):
    eng = gp.engine()
    pts = _points(base_points, n, n)
    es = _scalars(shape, n, random.Random(1000 * n + 10 * c + rows))
    want = _want(pts, es)
    d_s = eng.upload(_raw(es))
    try:
        with _Fixed(eng, pts, c, rows) as fx:
            assert fx.msm_dev(d_s, n) == want
            assert fx.msm_bytes(_raw(es), n) == want              # the host-pointer form
    finally:
        d_s.free()


@pytest.mark.parametrize("c,rows", [(16, 16), (13, 3), (10, 26), (16, 1)])
def test_every_digit_edge_value(gp, base_points, c, rows):
    """All of digit_edges' values in one MSM, one point each, and each value alone against its own point."""
    eng = gp.engine()
    vals = _digit_edge_values()
    pts = _points(base_points, len(vals), 3)
    with _Fixed(eng, pts, c, rows) as fx:
        assert fx.msm_bytes(_raw(vals), len(vals)) == _want(pts, vals)
        singles = cbind.ec_mul_batch(pts[:1] * len(vals), vals)
        for v, w in zip(vals, singles):
            assert fx.msm_bytes(_raw([v]), 1) == cbind.pack_points([w]), hex(v)


# ---- prefixes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,rows", [(16, 4), (13, 20), (16, 1)])
def test_fewer_scalars_than_points(gp, base_points, c, rows):
    eng = gp.engine()
    n = 1000
    pts = _points(base_points, n, 17)
    es = _scalars("uniform", n, random.Random(c * rows))
    d_s = eng.upload(_raw(es))
    try:
        with _Fixed(eng, pts, c, rows) as fx:
            for m in (0, 1, n - 1, n):
                want = _want(pts, es, m)
                assert fx.msm_dev(d_s, m) == want, m
                assert fx.msm_bytes(_raw(es[:m]), m) == want, m
            assert _want(pts, es, 0) == bytes(64)
    finally:
        d_s.free()


# ---- degenerate points --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,rows", [(16, 16), (13, 3)])
def test_degenerate_points(gp, base_points, c, rows):
    eng = gp.engine()
    n = 300
    rnd = random.Random(n + c)
    es = _scalars("uniform", n, rnd)
    same = [base_points[5]] * n
    with _Fixed(eng, same, c, rows) as fx:
        assert fx.msm_bytes(_raw(es), n) == _want(same, es)
    pairs, eq = [], []
    for i in range(n // 2):
        p = base_points[i]
        pairs += [p, OP(p.x, OC.p - p.y)]
        eq += [es[i], es[i]]
    with _Fixed(eng, pairs, c, rows) as fx:
        assert fx.msm_bytes(_raw(eq), n) == bytes(64) == _want(pairs, eq)
        assert fx.msm_bytes(_raw(es), n) == _want(pairs, es) != bytes(64)
    with _Fixed(eng, [INF] * n, c, rows) as fx:
        assert fx.msm_bytes(_raw(es), n) == bytes(64)
        assert fx.table_bytes(fx.info["rows"] - 1, 0, n) == bytes(64 * n)


# ---- skew: one bucket with tens of thousands of entries -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def skew(gp, base_points):
    """20 000 points under (16, 16): 320 000 virtual pairs, above the in-block sort's 2^17 -- the heavy-partition tile kernels run."""
    eng = gp.engine()
    n = 20000
    pts = _points(base_points, n, 1)
    d_p = eng.upload(cbind.pack_points(pts))
    fx = eng.fixed_base_create(d_p, n, 16, 16)
    cases = {}
    for shape in ("all_same", "bits01"):
        es = _scalars(shape, n, random.Random(n))
        cases[shape] = (eng.upload(_raw(es)), _want(pts, es))
    yield eng, fx, d_p, n, cases
    fx.close()
    d_p.free()
    for d_s, _ in cases.values():
        d_s.free()


@pytest.mark.parametrize("shape", ["all_same", "bits01"])
def test_skewed_scalars(skew, shape):
    eng, fx, d_p, n, cases = skew
    d_s, want = cases[shape]
    try:
        assert fx.msm_dev(d_s, n) == want
        assert eng.msm_runs_state()["planned"] is False           # a window group: the accumulation by runs only under "accum_runs" = 2
        assert eng.msm_dev(d_p, d_s, n) == want
        eng.set_option("accum_runs", 2)
        for cap, long_run in ((1 << 20, False), (1, True)):      # either side of the cap: k_accum_runs, the chunked accumulation
            eng.set_option("accum_runs_cap", cap)
            assert fx.msm_dev(d_s, n) == want, cap
            st = eng.msm_runs_state()
            assert st["planned"] is True and st["long_run"] is long_run, (cap, st)
    finally:
        _reset(eng)


# ---- size ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,rows", [(16, 16), (16, 4)])
def test_two_to_the_16(gp, base_points, c, rows):
    eng = gp.engine()
    n = 1 << 16
    pts = _points(base_points, n, 2)
    es = _scalars("uniform", n, random.Random(rows))
    d_p, d_s = eng.upload(cbind.pack_points(pts)), eng.upload(_raw(es))
    try:
        fx = eng.fixed_base_create(d_p, n, c, rows)
        got = fx.msm_dev(d_s, n)
        fx.close()
        assert got == eng.msm_dev(d_p, d_s, n) and got == _want(pts, es)
    finally:
        d_p.free()
        d_s.free()


def test_two_to_the_19_at_the_index_bound(gp, base_points):
    """(16, 16) over 2^19 points: 2^23 virtual pairs, the largest index the sorted entry holds."""
    eng = gp.engine()
    n = 1 << 19
    pb = cbind.pack_points(base_points)
    pb = (pb * (n // len(base_points) + 1))[:64 * n]
    rnd = random.Random(19)
    sb = rnd.randbytes(32 * n)
    d_p, d_s = eng.upload(pb), eng.upload(sb)
    try:
        fx = eng.fixed_base_create(d_p, n, 16, 16)
        assert fx.info["rows"] == 16 and fx.info["table_bytes"] == 64 << 23
        got = fx.msm_dev(d_s, n)
        fx.close()
        assert got == eng.msm_dev(d_p, d_s, n) and got != bytes(64)
    finally:
        d_p.free()
        d_s.free()


# ---- the asynchronous pair ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [0, 1])
def test_three_slots_two_objects_and_an_ordinary_msm_between(gp, base_points, lanes):
    eng = gp.engine()
    lib, ctx = eng.lib, eng.ctx
    n = 5000
    pts, pts2 = _points(base_points, n, 4), _points(base_points, 700, 9)
    rnd = random.Random(5000 + lanes)
    vecs = [_scalars(s, n, rnd) for s in ("uniform", "digit_edges", "top_window_edges")]
    wants = [_want(pts, es) for es in vecs]
    assert len(set(wants)) == 3
    bufs = [eng.upload(_raw(es)) for es in vecs]
    out = ctypes.create_string_buffer(64)
    try:
        eng.set_option("async_lanes", lanes)
        with _Fixed(eng, pts, 16, 4) as fx, _Fixed(eng, pts2, 13, 20) as fx2:
            sync = [fx.msm_dev(b, n) for b in bufs]
            assert sync == wants
            for slot in range(3):
                fx.msm_dev_enqueue(slot, bufs[slot], n)
            assert lib.bpmi_msm_fixed_dev_enqueue(fx.handle, 1, bufs[0].ptr, n) == -5 and b"pending" in lib.bpmi_last_error(ctx)      # a busy slot
            assert lib.bpmi_msm_fixed_dev_enqueue(fx2.handle, 1, bufs[0].ptr, 700) == -5
            assert lib.bpmi_msm_fixed_dev(fx.handle, bufs[0].ptr, n, out) == -5                                                     # the synchronous call needs slot 0
            assert [eng.msm_finish(slot) for slot in range(3)] == wants
            assert lib.bpmi_msm_finish(ctx, 0, out) == -5                                                                           # nothing enqueued any more
            # an ordinary MSM between two fixed calls, two objects alive on one ctx
            fx.msm_dev_enqueue(0, bufs[1], n)
            assert eng.msm_finish(0) == wants[1]
            assert eng.msm_bytes(cbind.pack_points(pts2), _raw(vecs[0][:700]), 700) == _want(pts2, vecs[0], 700)
            fx2.msm_dev_enqueue(1, bufs[2], 700)
            fx.msm_dev_enqueue(0, bufs[0], n - 1)
            assert eng.msm_finish(1) == _want(pts2, vecs[2], 700)
            assert eng.msm_finish(0) == _want(pts, vecs[0], n - 1)
            fx.msm_dev_enqueue(2, None, 0)                                                                                          # no scalars: the identity
            assert eng.msm_finish(2) == bytes(64)
    finally:
        _reset(eng)
        for b in bufs:
            b.free()


# ---- the automatic rule ---------------------------------------------------------------------------------------------------------------
def test_automatic_gives_the_same_bytes_and_the_plans_shape(gp, base_points, tmp_path):
    eng = gp.engine()
    exe = str(tmp_path / "msm_fixed_plan_main")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(REPO, "python-bulletproofs_amd", "csrc"),
                           os.path.join(REPO, "tests", "csrc_host", "msm_fixed_plan_main.cpp"), "-o", exe])
    for n in (300, 6000, 1 << 14):
        pts = _points(base_points, n, 6)
        es = _scalars("uniform", n, random.Random(n))
        want = _want(pts, es)
        plan = json.loads(subprocess.run([exe, "1", "0", str(n), "0", "0"], capture_output=True, text=True, check=True).stdout)
        with _Fixed(eng, pts, 0, 0) as fx:
            info = fx.info
            assert (info["n"], info["window_bits"], info["windows"], info["rows"], info["virtual_windows"], info["table_bytes"]) == \
                (n, plan["c"], plan["W"], plan["R"], plan["Wv"], plan["table_bytes"])
            assert info["rows"] * n <= 1 << 23
            assert fx.msm_bytes(_raw(es), n) == want
        with _Fixed(eng, pts, 16, 0) as fx:                       # automatic rows around explicit window bits
            assert fx.info["window_bits"] == 16 and fx.msm_bytes(_raw(es), n) == want


# ---- errors -------------------------------------------------------------------------------------------------------------------------------
def test_refusals(gp, base_points):
    eng = gp.engine()
    lib, ctx = eng.lib, eng.ctx
    n, pos = 70, 41
    pts = _points(base_points, n)
    good = cbind.pack_points(pts)
    G = OC.G
    bad = good[:64 * pos] + G.x.to_bytes(32, "little") + (G.y + 1).to_bytes(32, "little") + good[64 * pos + 64:]
    h = ctypes.c_void_p(1)
    err = lambda: lib.bpmi_last_error(ctx)
    d_bad = eng.upload(bad)
    try:
        # a point off the curve names its index; no object comes back
        assert lib.bpmi_fixed_base_create(ctx, bad, n, 16, 4, ctypes.byref(h)) == -3 and h.value is None
        assert b"bpmi_fixed_base_create: pts[%d] is not a point of the curve" % pos in err()
        eng.set_option("validate_points", 0)
        assert lib.bpmi_fixed_base_create(ctx, bad, n, 16, 4, ctypes.byref(h)) == 0 and h.value
        lib.bpmi_fixed_base_destroy(h)
        eng.set_option("validate_points", 1)
        assert lib.bpmi_fixed_base_create_dev(ctx, d_bad.ptr, n, 16, 4, ctypes.byref(h)) == 0 and h.value      # level 1: device pointers are the caller's
        lib.bpmi_fixed_base_destroy(h)
        eng.set_option("validate_points", 2)
        assert lib.bpmi_fixed_base_create_dev(ctx, d_bad.ptr, n, 16, 4, ctypes.byref(h)) == -3 and h.value is None
        assert b"bpmi_fixed_base_create_dev: pts[%d] is not a point of the curve" % pos in err()
        eng.set_option("validate_points", 1)
        # the bounds, refused before anything is read: the pointer is never followed
        for args, text in (((0, 16, 4), b"n must be at least 1"), (((1 << 26) + 1, 16, 1), b"BPMI_MAX_N"), ((70, 9, 1), b"window_bits must be 0 or 10 .. 16"),
                           ((70, 17, 1), b"window_bits must be 0 or 10 .. 16"), ((70, 16, 17), b"rows must be 0 or 1 .. W"), ((70, 13, 21), b"rows must be 0 or 1 .. W"),
                           (((1 << 19) + 1, 16, 16), b"n x rows exceeds 2^23"), (((1 << 23) + 1, 0, 0), b"n x rows exceeds 2^23")):
            assert lib.bpmi_fixed_base_create_dev(ctx, 64, args[0], args[1], args[2], ctypes.byref(h)) == -3 and text in err(), args
            assert lib.bpmi_fixed_base_create(ctx, ctypes.c_char_p(64), args[0], args[1], args[2], ctypes.byref(h)) == -3 and text in err(), args
        assert lib.bpmi_fixed_base_create(ctx, None, n, 16, 4, ctypes.byref(h)) == -3 and b"null" in err()
        assert lib.bpmi_fixed_base_create_dev(ctx, None, n, 16, 4, ctypes.byref(h)) == -3 and b"null" in err()
        assert lib.bpmi_fixed_base_create(ctx, good, n, 16, 4, None) == -3 and b"null" in err()
        out = ctypes.create_string_buffer(b"\x55" * 64, 64)
        with _Fixed(eng, pts, 16, 4, host=True) as fx:
            sb = _raw(range(1, n + 2))
            assert lib.bpmi_msm_fixed(fx.handle, sb, n + 1, out) == -3 and b"n_scalars exceeds" in err()
            assert lib.bpmi_msm_fixed_dev(fx.handle, d_bad.ptr, n + 1, out) == -3 and lib.bpmi_msm_fixed_dev_enqueue(fx.handle, 0, d_bad.ptr, n + 1) == -3
            assert lib.bpmi_msm_fixed(fx.handle, None, n, out) == -3 and lib.bpmi_msm_fixed(fx.handle, sb, n, None) == -3
            assert lib.bpmi_msm_fixed_dev_enqueue(fx.handle, 3, d_bad.ptr, n) == -3 and b"slot" in err()
            assert out.raw == b"\x55" * 64                         # refused before anything is written
            assert lib.bpmi_msm_fixed(fx.handle, sb, n, out) == 0 and out.raw == _want(pts, list(range(1, n + 1)))
            assert lib.bpmi_msm_fixed(fx.handle, None, 0, out) == 0 and out.raw == bytes(64)
        assert lib.bpmi_msm_fixed(None, b"", 0, out) == -3 and lib.bpmi_fixed_base_info(None, None) == -3
        lib.bpmi_fixed_base_destroy(None)
    finally:
        _reset(eng)
        d_bad.free()


# ---- the Python surface and the C example ---------------------------------------------------------------------------------------------------
def test_fixed_base_points_and_vector_commitment_fixed(gp, base_points):
    from bulletproofs_amd.pippenger import FixedBasePoints, PipSECP256k1
    from bulletproofs_amd.utils import vector_commitment, vector_commitment_fixed
    n = 150
    g, h = gp.to_gpu_list(_points(base_points, n, 9)), gp.to_gpu_list(_points(base_points, n, 400))
    rnd = random.Random(150)
    a, b = [rnd.randrange(Q) for _ in range(n)], [-(i + 1) for i in range(n)]
    for c, rows in ((16, 4), (0, 0)):
        fx = FixedBasePoints(g + h, c, rows)
        try:
            assert fx.n == 2 * n == len(fx) and fx.info["n"] == 2 * n
            got = PipSECP256k1.multiexp(fx, a + b)
            want = PipSECP256k1.multiexp(g + h, a + b)
            assert (got.x, got.y) == (want.x, want.y) and gp.same_point(got, cbind.msm(_points(base_points, n, 9) + _points(base_points, n, 400), a + b))
            vc, vw = vector_commitment_fixed(fx, a, b), vector_commitment(g, h, a, b)
            assert (vc.x, vc.y) == (vw.x, vw.y) == (want.x, want.y)
            short = fx.multiexp(a[:40])                           # the first 40 generators of the list
            ws = PipSECP256k1.multiexp(g[:40], a[:40])
            assert (short.x, short.y) == (ws.x, ws.y)
            with pytest.raises(Exception, match="Different number of group elements and exponents"):
                PipSECP256k1.multiexp(fx, a)
            with pytest.raises(Exception, match="More exponents"):
                fx.multiexp(a + b + [1])
        finally:
            fx.close()


def test_c_example(tmp_path):
    """examples/msm_fixed_c_abi.c: create, two MSMs in flight through the asynchronous pair, compared with bpmi_msm."""
    libdir = os.path.join(REPO, "python-bulletproofs_amd")
    exe = str(tmp_path / "msm_fixed_c_abi")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-I", os.path.join(REPO, "include"), os.path.join(REPO, "examples", "msm_fixed_c_abi.c"),
                           "-o", exe, os.path.join(libdir, "libbpmi.so"), "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"])
    r = subprocess.run([exe, "12", "16", "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "against bpmi_msm: ok" in r.stdout, r.stdout + r.stderr
