"""GPU parity of the batched MSM -- n_vec scalar vectors over ONE shared point set, n_vec points (bpmi_msm_batch, bpmi_msm_batch_dev,
bpmi_msm_batch_dev_enqueue; Pippenger.multiexp_batch, vector_commitment_batch) -- which replaces a loop of Pippenger.multiexp
(src/pippenger/pippenger.py:22-61) or of vector_commitment (src/utils/commitments.py:13).  Every row of
every batch is compared bit for bit with the C oracle's MSM of that row; the rows of a batch are all different, so a wrong row stride
cannot pass.  The routes (option "msm_batch_route") are forced: the tests do not depend on the measured bounds of the automatic plan."""
import ctypes
import random

import pytest

from helpers import Q
from oracle import cbind
from oracle.ec import INF, Point as OP, secp256k1 as OC

pytestmark = pytest.mark.gpu

LIGHT, MID, LOOP = 1, 2, 3
HALF = (Q - 1) // 2


@pytest.fixture(scope="module")
def gp():
    import gpu_common
    return gpu_common


@pytest.fixture(scope="module")
def base_points(gp):
    """1 000 distinct points, repeated to the size a case needs (the oracle's cost is the scalars')."""
    return gp.rand_points(1000, 97)[0]


def _points(base, n, shift=0):
    return [base[(i + shift) % len(base)] for i in range(n)]


def _raw(es):
    """32 bytes little-endian each, NOT reduced: the library reduces on load."""
    return b"".join(int(e).to_bytes(32, "little") for e in es)


def _scalars(shape, n, rnd):
    """The shapes of tests/test_gpu_msm_midsize.py, and the rows of this file's own."""
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
    if shape == "top_heavy":
        return [(0x5A5A << 240) | rnd.randrange(1 << 240) for _ in range(n)]
    if shape == "zeros":
        return [0] * n
    if shape == "above_q":                     # any 256-bit value is allowed: [q, 2^256)
        return [rnd.choice((Q, Q + 1, (1 << 256) - 1, 2 * Q - 1 if 2 * Q - 1 < 1 << 256 else Q + 5, rnd.randrange(Q, 1 << 256))) for _ in range(n)]
    if shape == "edges":
        vals = [0, 1, Q - 1, HALF, HALF + 1]
        return [vals[(i + rnd.randrange(2)) % len(vals)] for i in range(n)]
    raise ValueError(shape)


def _want(seg_pts, rows):
    """rows[v][s] = the scalars of row v in segment s; the oracle's MSM of every row over the concatenated segments"""
    pb = b"".join(cbind.pack_points(p) for p in seg_pts)
    total = sum(len(p) for p in seg_pts)
    return [cbind.msm_bytes(pb, cbind.pack_scalars([e for seg in row for e in seg]), total) for row in rows]


def _matrices(rows, nseg):
    return [b"".join(_raw(row[s]) for row in rows) for s in range(nseg)]


class _Dev:
    """The segments of a batch in device memory, freed at the end of the `with`."""

    def __init__(self, eng, seg_pts, rows):
        self.eng, self.nseg, self.n_vec = eng, len(seg_pts), len(rows)
        self.ns = [len(p) for p in seg_pts]
        mats = _matrices(rows, self.nseg)
        self.bufs = [eng.upload(cbind.pack_points(p)) if p else None for p in seg_pts] + [eng.upload(m) if m else None for m in mats]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.bufs:
            if b is not None:
                b.free()

    def run(self, d_out=None):
        return self.eng.msm_batch_dev(self.bufs[:self.nseg], self.ns, self.bufs[self.nseg:], self.n_vec, d_out)

    def arrays(self):
        P = (ctypes.c_void_p * self.nseg)(*[b.ptr if b is not None else None for b in self.bufs[:self.nseg]])
        S = (ctypes.c_void_p * self.nseg)(*[b.ptr if b is not None else None for b in self.bufs[self.nseg:]])
        return P, (ctypes.c_uint64 * self.nseg)(*self.ns), S


def _split(buf):
    return [buf[i: i + 64] for i in range(0, len(buf), 64)]


def _reset(eng):
    eng.set_option("msm_batch_route", 0)
    eng.set_option("msm_batch_vecs", 0)
    eng.set_option("validate_points", 1)


def _rows(total_by_seg, n_vec, seed, shape="uniform"):
    rnd = random.Random(seed)
    return [[_scalars(shape, n, rnd) for n in total_by_seg] for _ in range(n_vec)]


# ---- routes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,total", [(LIGHT, 1), (LIGHT, 2), (LIGHT, 129), (LIGHT, 512), (MID, 513), (MID, 8448), (MID, 8449), (MID, 33792), (LOOP, 33793)])
def test_forced_route_at_its_edges(gp, base_points, route, total):
    """LIGHT up to 512 pairs; MID with one part up to 8 448, two from 8 449, four at 33 792; the loop above.  Three different rows."""
    eng = gp.engine()
    pts = [_points(base_points, total)]
    rows = _rows([total], 3, total)
    want = _want(pts, rows)
    assert len(set(want)) == 3
    try:
        eng.set_option("msm_batch_route", route)
        with _Dev(eng, pts, rows) as d:
            assert _split(d.run()) == want
    finally:
        _reset(eng)


@pytest.mark.parametrize("total,n_vec,routes", [(512, 32, (LIGHT, MID, LOOP)), (513, 32, (MID, LOOP)), (25344, 64, (MID, LOOP)), (25345, 64, (MID, LOOP)),
                                                (33792, 4, (MID, LOOP)), (33793, 4, (LOOP,))])
def test_automatic_route_agrees_with_its_neighbours(gp, base_points, total, n_vec, routes):
    """Either side of every size at which the automatic plan changes its route (with enough vectors for it to leave the loop: 32, and 64 at
    three blocks per window) and of the largest size a forced MID holds, against the oracle and against every route that holds the size."""
    eng = gp.engine()
    pts = [_points(base_points, total, 5)]
    rows = _rows([total], n_vec, total + 1)
    want = _want(pts, rows)
    try:
        with _Dev(eng, pts, rows) as d:
            assert _split(d.run()) == want                          # whatever the plan picks
            for r in routes:
                eng.set_option("msm_batch_route", r)
                assert _split(d.run()) == want, r
    finally:
        _reset(eng)


# ---- segments ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [(64, 64, 1), (0, 5, 0), (300, 300)])
def test_segments(gp, base_points, ns):
    """(64, 64, 1): the statement P = <a, g> + <b, h> + c u; an empty first and last segment; two matrices with their own row strides."""
    eng = gp.engine()
    pts = [_points(base_points, n, 100 * s) for s, n in enumerate(ns)]
    rows = _rows(ns, 5, sum(ns))
    want = _want(pts, rows)
    assert len(set(want)) == 5
    try:
        with _Dev(eng, pts, rows) as d:
            for r in (0, LIGHT if sum(ns) <= 512 else MID, LOOP):
                eng.set_option("msm_batch_route", r)
                assert _split(d.run()) == want, r
    finally:
        _reset(eng)


@pytest.mark.parametrize("route,n", [(LIGHT, 129), (MID, 700), (0, 129)])
def test_host_pointer_form(gp, base_points, route, n):
    eng = gp.engine()
    pts = [_points(base_points, n, 3)]
    rows = _rows([n], 6, n + route)
    want = _want(pts, rows)
    try:
        eng.set_option("msm_batch_route", route)
        assert _split(eng.msm_batch_bytes(cbind.pack_points(pts[0]), _matrices(rows, 1)[0], n, 6)) == want
    finally:
        _reset(eng)


# ---- the number of vectors ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many_rows(base_points):
    """65 rows of 33 pairs and their values: the n_vec cases are prefixes of them."""
    pts = [_points(base_points, 33, 11)]
    rows = _rows([33], 65, 65)
    return pts, rows, _want(pts, rows)


@pytest.mark.parametrize("route", [LIGHT, MID])
@pytest.mark.parametrize("n_vec", [1, 2, 3, 64, 65])
def test_vector_counts_around_the_tails_wave_boundary(gp, many_rows, n_vec, route):
    eng = gp.engine()
    pts, rows, want = many_rows
    try:
        eng.set_option("msm_batch_route", route)
        with _Dev(eng, pts, rows[:n_vec]) as d:
            assert _split(d.run()) == want[:n_vec]
    finally:
        _reset(eng)


@pytest.mark.parametrize("route,total", [(LIGHT, 129), (MID, 8449)])
def test_row_ranges_of_three_vectors_per_launch(gp, base_points, route, total):
    """7 vectors at 3 per launch: three launches, the last one short, all on one region of window sums."""
    eng = gp.engine()
    pts = [_points(base_points, total, 7)]
    rows = _rows([total], 7, total + 7)
    want = _want(pts, rows)
    try:
        eng.set_option("msm_batch_route", route)
        with _Dev(eng, pts, rows) as d:
            whole = d.run()
            eng.set_option("msm_batch_vecs", 3)
            assert _split(d.run()) == want and _split(whole) == want
    finally:
        _reset(eng)


# ---- scalar shapes, one per row ------------------------------------------------------------------------------------------------
SHAPES = ["uniform", "zeros", "all_same", "bits01", "top_window_edges", "top_heavy", "above_q", "edges"]


@pytest.mark.parametrize("route,ns", [(LIGHT, (129,)), (LIGHT, (200, 312)), (MID, (8449,)), (MID, (513, 1, 700))])
def test_scalar_shapes_per_row(gp, base_points, route, ns):
    """Row 1 is all zeros between rows that are not; a row of values in [q, 2^256); a row of 0, 1, q - 1, (q +- 1) / 2."""
    eng = gp.engine()
    pts = [_points(base_points, n, 31 * s) for s, n in enumerate(ns)]
    rnd = random.Random(sum(ns))
    rows = [[_scalars(shape, n, rnd) for n in ns] for shape in SHAPES]
    want = _want(pts, rows)
    assert want[1] == bytes(64) and want[0] != bytes(64) and want[2] != bytes(64)
    try:
        eng.set_option("msm_batch_route", route)
        with _Dev(eng, pts, rows) as d:
            assert _split(d.run()) == want
    finally:
        _reset(eng)


@pytest.mark.parametrize("route,n", [(LIGHT, 130), (MID, 8460), (LOOP, 130)])
def test_a_row_whose_terms_cancel(gp, base_points, route, n):
    """Points [P, -P, identity, P', -P', identity, ...]; row 1 gives P and -P the same scalar: 64 zero bytes beside non-zero neighbours."""
    eng = gp.engine()
    pts = []
    for i in range(n):
        p = base_points[(i // 3) % len(base_points)]
        pts.append(p if i % 3 == 0 else (OP(p.x, OC.p - p.y) if i % 3 == 1 else INF))
    rnd = random.Random(n)
    cancel = []
    for i in range(n):
        cancel.append(cancel[-1] if i % 3 == 1 else rnd.randrange(Q))
    if n % 3 == 1:
        cancel[-1] = 0                                                   # (a last P without its -P)
    rows = [[_scalars("uniform", n, rnd)], [cancel], [_scalars("uniform", n, rnd)]]
    want = _want([pts], rows)
    assert want[1] == bytes(64) and want[0] != bytes(64) and want[2] != bytes(64)
    try:
        eng.set_option("msm_batch_route", route)
        with _Dev(eng, [pts], rows) as d:
            assert _split(d.run()) == want
    finally:
        _reset(eng)


# ---- the enqueue form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,ns", [(LIGHT, (64, 64, 1)), (MID, (600, 0, 77)), (LOOP, (40,))])
def test_enqueue_form_is_ordered_on_the_ctx_stream(gp, base_points, route, ns):
    eng = gp.engine()
    pts = [_points(base_points, n, 13 * s) for s, n in enumerate(ns)]
    rows = _rows(ns, 5, sum(ns) + 2)
    d_out, d_copy = eng.upload(b"\x55" * 320), eng.upload(b"\xAA" * 320)
    try:
        eng.set_option("msm_batch_route", route)
        with _Dev(eng, pts, rows) as d:
            sync = d.run()
            assert _split(sync) == _want(pts, rows)
            assert d.run(d_out) is None
            eng._ck(eng.lib.bpmi_memcpy_dev(eng.ctx, d_copy.ptr, d_out.ptr, 320))       # queued behind it on the same ctx
            eng.sync()
            assert d_copy.download(320) == sync and d_out.download(320) == sync
    finally:
        _reset(eng)
        d_out.free()
        d_copy.free()


def test_no_pairs_and_no_vectors(gp, base_points):
    eng = gp.engine()
    lib, ctx = eng.lib, eng.ctx
    out = ctypes.create_string_buffer(b"\x55" * 192, 192)
    P, S, N = (ctypes.c_void_p * 2)(None, None), (ctypes.c_void_p * 2)(None, None), (ctypes.c_uint64 * 2)(0, 0)
    assert lib.bpmi_msm_batch_dev(ctx, 2, P, N, S, 3, out) == 0 and out.raw == bytes(192)           # no pairs: n_vec identities
    out = ctypes.create_string_buffer(b"\x55" * 192, 192)
    assert lib.bpmi_msm_batch(ctx, None, 0, None, 3, out) == 0 and out.raw == bytes(192)
    out = ctypes.create_string_buffer(b"\x55" * 192, 192)
    N5 = (ctypes.c_uint64 * 2)(5, 5)
    assert lib.bpmi_msm_batch_dev(ctx, 2, P, N5, S, 0, out) == 0 and out.raw == b"\x55" * 192       # no vectors: nothing is touched
    assert lib.bpmi_msm_batch(ctx, None, 0, None, 0, out) == 0 and out.raw == b"\x55" * 192
    d_out = eng.upload(b"\x55" * 192)
    try:
        assert lib.bpmi_msm_batch_dev_enqueue(ctx, 2, P, N, S, 3, d_out.ptr) == 0
        eng.sync()
        assert d_out.download(192) == bytes(192)
    finally:
        d_out.free()


# ---- errors through the C ABI -----------------------------------------------------------------------------------------------------
def test_argument_caps_and_their_messages(gp, base_points):
    eng = gp.engine()
    lib, ctx = eng.lib, eng.ctx
    pts = [_points(base_points, 20)]
    rows = _rows([20], 2, 20)
    out = ctypes.create_string_buffer(b"\x55" * 128, 128)
    with _Dev(eng, pts, rows) as d:
        P, N, S = d.arrays()
        err = lambda: lib.bpmi_last_error(ctx)
        for nseg in (0, 4):
            assert lib.bpmi_msm_batch_dev(ctx, nseg, P, N, S, 2, out) == -3 and b"nseg must be 1 .. 3" in err()
            assert lib.bpmi_msm_batch_dev_enqueue(ctx, nseg, P, N, S, 2, d.bufs[0].ptr) == -3 and b"nseg must be 1 .. 3" in err()
        for args in ((None, N, S, out), (P, None, S, out), (P, N, None, out), (P, N, S, None)):
            assert lib.bpmi_msm_batch_dev(ctx, 1, args[0], args[1], args[2], 2, args[3]) == -3 and b"null" in err()
        Pn = (ctypes.c_void_p * 1)(None)
        assert lib.bpmi_msm_batch_dev(ctx, 1, Pn, N, S, 2, out) == -3 and b"null segment" in err()
        assert lib.bpmi_msm_batch(ctx, None, 20, b"", 2, out) == -3 and b"null" in err()
        big = (ctypes.c_uint64 * 1)((1 << 26) + 1)
        assert lib.bpmi_msm_batch_dev(ctx, 1, P, big, S, 1, out) == -3 and b"BPMI_MAX_N" in err()
        assert lib.bpmi_msm_batch(ctx, b"", (1 << 26) + 1, b"", 1, out) == -3 and b"BPMI_MAX_N" in err()
        assert lib.bpmi_msm_batch_dev(ctx, 1, P, N, S, (1 << 20) + 1, out) == -3 and b"2^20 vectors" in err()
        n1025 = (ctypes.c_uint64 * 1)(1025)
        assert lib.bpmi_msm_batch_dev(ctx, 1, P, n1025, S, 1 << 20, out) == -3 and b"2^30 pairs" in err()
        assert lib.bpmi_msm_batch_dev_enqueue(ctx, 1, P, n1025, S, 1 << 20, d.bufs[0].ptr) == -3 and b"2^30 pairs" in err()
        assert out.raw == b"\x55" * 128                                          # refused before anything is written
        try:
            n513 = (ctypes.c_uint64 * 1)(513)
            eng.set_option("msm_batch_route", LIGHT)
            assert lib.bpmi_msm_batch_dev(ctx, 1, P, n513, S, 2, out) == -3 and b"LIGHT" in err() and b"512 pairs" in err()
            eng.set_option("msm_batch_route", MID)
            n33793 = (ctypes.c_uint64 * 1)(33793)
            assert lib.bpmi_msm_batch_dev(ctx, 1, P, n33793, S, 2, out) == -3 and b"MID" in err() and b"33792 pairs" in err()
            assert lib.bpmi_set_option(ctx, b"msm_batch_route", 4) == -3
            assert lib.bpmi_set_option(ctx, b"msm_batch_vecs", -1) == -3
        finally:
            _reset(eng)
        assert lib.bpmi_msm_batch_dev(ctx, 1, P, N, S, 2, out) == 0 and _split(out.raw) == _want(pts, rows)


@pytest.mark.parametrize("route", [LIGHT, MID, LOOP])
def test_off_curve_points_are_named_and_the_results_zeroed(gp, base_points, route):
    eng = gp.engine()
    lib, ctx = eng.lib, eng.ctx
    n, n_vec, pos = 70, 3, 41
    good = cbind.pack_points(_points(base_points, n))
    G = OC.G
    bad = good[:64 * pos] + G.x.to_bytes(32, "little") + (G.y + 1).to_bytes(32, "little") + good[64 * pos + 64:]
    rows = _rows([n], n_vec, 70)
    mat = _matrices(rows, 1)[0]
    out = ctypes.create_string_buffer(b"\x55" * 192, 192)
    d_p, d_s = eng.upload(bad), eng.upload(mat)
    try:
        eng.set_option("msm_batch_route", route)
        assert lib.bpmi_msm_batch(ctx, bad, n, mat, n_vec, out) == -3
        assert b"bpmi_msm_batch: pts[%d] is not a point of the curve" % pos in lib.bpmi_last_error(ctx) and out.raw == bytes(192)
        P, S, N = (ctypes.c_void_p * 2)(None, d_p.ptr), (ctypes.c_void_p * 2)(None, d_s.ptr), (ctypes.c_uint64 * 2)(0, n)
        out = ctypes.create_string_buffer(b"\x55" * 192, 192)
        assert lib.bpmi_msm_batch_dev(ctx, 2, P, N, S, n_vec, out) == 0                # level 1: device pointers are the caller's responsibility
        eng.set_option("validate_points", 2)
        assert lib.bpmi_msm_batch_dev(ctx, 2, P, N, S, n_vec, out) == -3
        assert b"bpmi_msm_batch_dev: d_pts[1][%d] is not a point of the curve" % pos in lib.bpmi_last_error(ctx) and out.raw == bytes(192)
        d_p.upload(good)
        assert lib.bpmi_msm_batch_dev(ctx, 2, P, N, S, n_vec, out) == 0 and _split(out.raw) == _want([_points(base_points, n)], rows)
        eng.set_option("validate_points", 1)
        assert lib.bpmi_msm_batch(ctx, good, n, mat, n_vec, out) == 0 and _split(out.raw) == _want([_points(base_points, n)], rows)
    finally:
        _reset(eng)
        d_p.free()
        d_s.free()


def test_a_pending_slot_refuses_the_call(gp, base_points):
    eng = gp.engine()
    lib, ctx = eng.lib, eng.ctx
    pts = [_points(base_points, 200)]
    rows = _rows([200], 4, 200)
    want = _want(pts, rows)
    out, one = ctypes.create_string_buffer(256), ctypes.create_string_buffer(64)
    with _Dev(eng, pts, rows) as d:
        P, N, S = d.arrays()
        single = cbind.msm_bytes(cbind.pack_points(pts[0]), cbind.pack_scalars(rows[0][0]), 200)
        try:
            for route in (LIGHT, LOOP):
                eng.set_option("msm_batch_route", route)
                assert lib.bpmi_msm_dev_enqueue(ctx, 0, d.bufs[0].ptr, d.bufs[1].ptr, 200) == 0
                assert lib.bpmi_msm_batch_dev(ctx, 1, P, N, S, 4, out) == -5 and b"pending" in lib.bpmi_last_error(ctx)
                assert lib.bpmi_msm_batch_dev_enqueue(ctx, 1, P, N, S, 4, d.bufs[1].ptr) == -5
                assert lib.bpmi_msm_batch(ctx, cbind.pack_points(pts[0]), 200, _matrices(rows, 1)[0], 4, out) == -5
                assert lib.bpmi_msm_finish(ctx, 0, one) == 0 and one.raw == single       # the pending MSM is left alone
                assert lib.bpmi_msm_batch_dev(ctx, 1, P, N, S, 4, out) == 0 and _split(out.raw) == want
        finally:
            _reset(eng)


# ---- the Python surface -----------------------------------------------------------------------------------------------------------
def test_multiexp_batch_with_a_list_and_with_device_points(gp, base_points):
    from bulletproofs_amd.pippenger import DevicePoints, PipSECP256k1
    n = 150
    opts = _points(base_points, n, 9)
    gs = gp.to_gpu_list(opts)
    rnd = random.Random(150)
    rows = [[rnd.randrange(Q) for _ in range(n)] for _ in range(4)] + [[-(i + 1) for i in range(n)], [Q + i for i in range(n)]]
    want = [cbind.msm(opts, r) for r in rows]
    got = PipSECP256k1.multiexp_batch(gs, rows)
    assert len(got) == 6 and all(gp.same_point(g, w) for g, w in zip(got, want))
    assert all(gp.same_point(g, PipSECP256k1.multiexp(gs, r)) for g, r in zip(got, rows))
    dev = DevicePoints(gs)
    got = PipSECP256k1.multiexp_batch(dev, rows)
    assert all(gp.same_point(g, w) for g, w in zip(got, want))
    with pytest.raises(Exception, match="Different number of group elements and exponents"):
        PipSECP256k1.multiexp_batch(dev, rows + [[1]])


def test_vector_commitment_batch_equals_the_loop(gp, base_points):
    from bulletproofs_amd.utils import vector_commitment, vector_commitment_batch
    n = 64
    g, h = gp.to_gpu_list(_points(base_points, n)), gp.to_gpu_list(_points(base_points, n, 500))
    rnd = random.Random(64)
    A = [[rnd.randrange(Q) for _ in range(n)] for _ in range(5)]
    B = [[rnd.randrange(Q) for _ in range(n)] for _ in range(5)]
    got = vector_commitment_batch(g, h, A, B)
    want = [vector_commitment(g, h, a, b) for a, b in zip(A, B)]
    assert len(got) == 5 and all(x.x == y.x and x.y == y.y for x, y in zip(got, want))
    assert len({(x.x, x.y) for x in got}) == 5
