"""GPU parity of the statements a batched inner-product prover makes from its tables (bpmi_ipa_batch_prover_commit_batch,
BatchInnerProductProver.commit / commit_packed): out[p] = sum a_p[j] g_j + sum b_p[j] (c_j h_j) + t_p u, byte for byte the C oracle's MSM
over [g | h | u] -- what a loop of vector_commitment(g, h, a, b) (src/utils/commitments.py:13) plus inner_product(a, b) * u gives --
for every vector length at which the scalar kernel takes another path, every u_mode, NULL halves, h_scale, table widths, scalars and
generators at their edges; the statements feed the prover and the packed batch verifier; the C ABI refuses what include/bpmi.h says.

Unless a test says otherwise the tables are built with 6-bit windows (180 MB at n = 1 024); every prover is closed in `finally`."""
import ctypes
import random

import pytest

from helpers import Q
from oracle import cbind

pytestmark = pytest.mark.gpu

E_ARG = -3


@pytest.fixture(scope="module")
def gp():
    import gpu_common
    return gpu_common


def _points(gp, count, seed):
    """count distinct valid points k_i G from the engine's batched multiplication"""
    from bulletproofs_amd.ec import secp256k1, unpack_points
    rnd = random.Random(seed)
    ks = b"".join(rnd.randrange(1, Q).to_bytes(32, "little") for _ in range(count))
    return unpack_points(gp.engine().ec_mul_batch_bytes(secp256k1.G.to_le64() * count, ks, count), count)


def _vectors(n, count, seed):
    rnd = random.Random(seed)
    return [[rnd.randrange(Q) for _ in range(n)] for _ in range(count)]


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b)) % Q


def _sc(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


class _Options:
    """engine options for the length of a test, restored afterwards"""

    def __init__(self, eng, **opts):
        self.eng, self.opts = eng, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.eng.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.eng.set_option(k, 0)


class _Oracle:
    """The C oracle's MSM over [g | h | u] with the scalars [a | b c | t]: the expected 64 bytes of one statement."""

    def __init__(self, g, h, u, scale=None):
        self.n, self.scale = len(g), scale
        self.pts = b"".join(p.to_le64() for p in list(g) + list(h) + [u])

    def one(self, a, b, t):
        n = self.n
        bc = list(b) if self.scale is None else [x * c % Q for x, c in zip(b, self.scale)]
        return cbind.msm_bytes(self.pts, _sc(list(a) + bc + [t % Q]), 2 * n + 1, threads=1 if n < 256 else None)

    def many(self, As, Bs, ts):
        return b"".join(self.one(a, b, t) for a, b, t in zip(As, Bs, ts))


def _prover(g, h, u, h_scale=None):
    from bulletproofs_amd.innerproduct import BatchInnerProductProver
    return BatchInnerProductProver(g, h, u, h_scale=h_scale)


# ---- 1. shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 4, 64, 128, 512, 1024])
def test_parity_across_shapes_and_modes(gp, n):
    """No tree (n = 1), a tree inside a wave, a whole wave, the meeting of the waves' sums in LDS (128), the NT = 512 and 1 024 kernels;
    a count one past a block boundary (a last block with one live proof) and count = 1; the three u_modes, mode 1 equal to mode 2 fed
    with the host's <a_p, b_p>."""
    per_block = (256 if n <= 256 else n) // n
    count = per_block + 1
    pts = _points(gp, 2 * n + 1, 2100 + n)
    g, h, u = pts[:n], pts[n: 2 * n], pts[2 * n]
    As, Bs = _vectors(n, count, 3 * n + 1), _vectors(n, count, 5 * n + 2)
    ts = [_dot(a, b) for a, b in zip(As, Bs)]
    orc = _Oracle(g, h, u)
    want0, want_t = orc.many(As, Bs, [0] * count), orc.many(As, Bs, ts)
    assert want0 != want_t
    with _Options(gp.engine(), prover_table_bits=6):
        bp = _prover(g, h, u)
        try:
            for m in (count, 1):
                assert bp.commit_packed(As[:m], Bs[:m]) == want0[: 64 * m], ("mode 0", m)
                assert bp.commit_packed(As[:m], Bs[:m], "inner") == want_t[: 64 * m], ("mode 1", m)
                assert bp.commit_packed(As[:m], Bs[:m], ts[:m]) == want_t[: 64 * m], ("mode 2", m)
            ms = bp.commit_last_ms()
            assert ms["device"] > 0 and ms["call"] >= ms["device"]
        finally:
            bp.close()


# ---- 2. h_scale --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 128])
def test_h_scale_goes_into_the_scalars_not_into_the_dot(gp, n):
    """The statement runs over c_j h_j; the dot of mode 1 is over the UNSCALED b: with these c_j the scaled dot is another number, and
    the statement made with it another point."""
    count = 3
    pts = _points(gp, 2 * n + 1, 2200 + n)
    g, h, u = pts[:n], pts[n: 2 * n], pts[2 * n]
    rnd = random.Random(22 + n)
    scale = [0, 1, Q - 1] + [rnd.randrange(2, Q) for _ in range(n - 3)]
    As, Bs = _vectors(n, count, 23), _vectors(n, count, 24)
    ts = [_dot(a, b) for a, b in zip(As, Bs)]
    scaled = [_dot(a, [x * c % Q for x, c in zip(b, scale)]) for a, b in zip(As, Bs)]
    assert all(t != s for t, s in zip(ts, scaled))
    orc = _Oracle(g, h, u, scale)
    want0, want_t, wrong = orc.many(As, Bs, [0] * count), orc.many(As, Bs, ts), orc.many(As, Bs, scaled)
    assert want0 != _Oracle(g, h, u).many(As, Bs, [0] * count)
    with _Options(gp.engine(), prover_table_bits=6):
        bp = _prover(g, h, u, h_scale=scale)
        try:
            assert bp.commit_packed(As, Bs) == want0
            got = bp.commit_packed(As, Bs, "inner")
            assert got == want_t and got != wrong
            assert bp.commit_packed(As, Bs, ts) == want_t
            assert bp.commit_packed(None, Bs) == orc.many([[0] * n] * count, Bs, [0] * count)
        finally:
            bp.close()


# ---- 3. table widths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [4, 13, 16])
def test_table_widths(gp, bits):
    """4-bit windows (64 per scalar), 13-bit (20, the top one short) and the default 16-bit tables (302 MB at n = 4): the same values."""
    n, count = 4, 5
    pts = _points(gp, 2 * n + 1, 2300)
    g, h, u = pts[:n], pts[n: 2 * n], pts[2 * n]
    As, Bs = _vectors(n, count, 31), _vectors(n, count, 32)
    ts = [_dot(a, b) for a, b in zip(As, Bs)]
    orc = _Oracle(g, h, u)
    with _Options(gp.engine(), prover_table_bits=bits):
        bp = _prover(g, h, u)
        try:
            assert bp.commit_packed(As, Bs) == orc.many(As, Bs, [0] * count)
            assert bp.commit_packed(As, Bs, "inner") == orc.many(As, Bs, ts)
        finally:
            bp.close()


# ---- 4. scalars at the edges -------------------------------------------------------------------------------------------------
W7FFF = int("7FFF" * 16, 16)                             # every 16-bit window 0x7FFF: the largest digit that stays positive below the half
W8000 = int("7FFF" + "8000" * 15, 16)                    # windows 0 .. 14 are 0x8000 = 2^(tw-1): the last positive digit, no carry
WFFFF = int("7FFE" + "FFFF" * 15, 16)                    # windows 0 .. 14 are 0xFFFF: digit -1 and a carry, all the way into the top window
EDGES = [0, 1, Q - 1, (Q - 1) // 2, (Q + 1) // 2, W7FFF, W8000, WFFFF, int("8000" * 16, 16), Q - W7FFF, Q - W8000, Q - WFFFF]


@pytest.mark.parametrize("bits", [6, 16])
def test_scalars_at_the_edges(gp, bits):
    """0, 1, q - 1 and the two neighbours of the fold to q - s; for the 16-bit table the magnitudes whose windows are 0x7FFF, 0x8000
    and 0xFFFF throughout (all three are below (q - 1) / 2, so the kernel walks them as they stand; q minus each walks the same
    windows negated).  Every edge value meets every other on g and h, and rides on u as t."""
    assert all(0 <= e < Q for e in EDGES) and all(e <= (Q - 1) // 2 for e in (W7FFF, W8000, WFFFF))
    n = 4
    pts = _points(gp, 2 * n + 1, 2400)
    g, h, u = pts[:n], pts[n: 2 * n], pts[2 * n]
    m = len(EDGES)
    As = [[EDGES[(i + j) % m] for j in range(n)] for i in range(m)] + [[0] * n]
    Bs = [[EDGES[(2 * i + 3 * j + 1) % m] for j in range(n)] for i in range(m)] + [[0] * n]
    count = m + 1
    ts = EDGES + [0]
    dots = [_dot(a, b) for a, b in zip(As, Bs)]
    orc = _Oracle(g, h, u)
    with _Options(gp.engine(), prover_table_bits=bits):
        bp = _prover(g, h, u)
        try:
            got0 = bp.commit_packed(As, Bs)
            assert got0 == orc.many(As, Bs, [0] * count)
            assert got0[-64:] == bytes(64)                                       # a = b = 0 without a u term: the identity
            assert bp.commit_packed(As, Bs, [0] * count) == got0                 # t = 0 is no u term
            assert bp.commit_packed(As, Bs, ts) == orc.many(As, Bs, ts)
            assert bp.commit_packed(As, Bs, "inner") == orc.many(As, Bs, dots)
        finally:
            bp.close()


# ---- 5. generators at the edges ----------------------------------------------------------------------------------------------
def test_degenerate_generators_and_a_cancellation(gp):
    """g_1 = g_0, h_0 = -g_0, g_2 = the identity (legal by the prover's contract): table rows that coincide, cancel or are empty.  Equal
    scalars on g_0 and on h_0 = -g_0, anything on the identity: the statement is the identity."""
    from bulletproofs_amd.ec import Point
    n, count = 4, 6
    pts = _points(gp, 2 * n + 1, 2500)
    g, h, u = pts[:n], pts[n: 2 * n], pts[2 * n]
    g[1] = g[0]
    h[0] = -g[0]
    g[2] = Point.IDENTITY_ELEMENT
    As, Bs = _vectors(n, count, 51), _vectors(n, count, 52)
    s = As[0][0]
    As[0], Bs[0] = [s, 0, As[0][2], 0], [s, 0, 0, 0]                             # s g_0 + x O - s g_0
    As[1], Bs[1] = [s, Q - s, 7, 0], [0, 0, 0, 0]                                # s g_0 - s g_1 with g_1 = g_0
    As[2] = [As[2][0]] * n                                                       # equal scalars on the coinciding generators
    ts = [_dot(a, b) for a, b in zip(As, Bs)]
    orc = _Oracle(g, h, u)
    with _Options(gp.engine(), prover_table_bits=6):
        bp = _prover(g, h, u)
        try:
            got0 = bp.commit_packed(As, Bs)
            assert got0 == orc.many(As, Bs, [0] * count)
            assert got0[:128] == bytes(128)
            assert bp.commit_packed(As, Bs, "inner") == orc.many(As, Bs, ts)
            assert [p.to_le64() for p in bp.commit(As[:2], Bs[:2])] == [Point.IDENTITY_ELEMENT.to_le64()] * 2
        finally:
            bp.close()


# ---- 6. NULL halves ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 128])
def test_null_halves_equal_zero_halves(gp, n):
    """a only and b only are the full call with the other half zero (and the oracle's value), with and without an explicit t."""
    count = 256 // n + 1
    pts = _points(gp, 2 * n + 1, 2600 + n)
    g, h, u = pts[:n], pts[n: 2 * n], pts[2 * n]
    As, Bs = _vectors(n, count, 61), _vectors(n, count, 62)
    ts = [random.Random(63).randrange(Q) for _ in range(count)]
    zero = [[0] * n] * count
    orc = _Oracle(g, h, u)
    with _Options(gp.engine(), prover_table_bits=6):
        bp = _prover(g, h, u)
        try:
            for t_arg, t_val in ((None, [0] * count), (ts, ts)):
                a_only, b_only = bp.commit_packed(As, None, t_arg), bp.commit_packed(None, Bs, t_arg)
                assert a_only == bp.commit_packed(As, zero, t_arg) == orc.many(As, zero, t_val)
                assert b_only == bp.commit_packed(zero, Bs, t_arg) == orc.many(zero, Bs, t_val)
        finally:
            bp.close()


# ---- 7. round trip -----------------------------------------------------------------------------------------------------------
def test_round_trip_through_the_prover_and_the_packed_verifier(gp):
    """commit() makes the statements prove1 takes, and those under which prove2's proofs verify; one statement moved by G fails the batch."""
    from bulletproofs_amd.ec import secp256k1
    from bulletproofs_amd.innerproduct import BatchInnerProductVerifier
    n, count = 64, 5
    pts = _points(gp, 2 * n + 1, 2700)
    g, h, u = pts[:n], pts[n: 2 * n], pts[2 * n]
    As, Bs = _vectors(n, count, 71), _vectors(n, count, 72)
    cs = [_dot(a, b) for a, b in zip(As, Bs)]
    seeds = [b"", b"a", b"bc", b"def", b"seed"]
    with _Options(gp.engine(), prover_table_bits=6):
        bp = _prover(g, h, u)
        try:
            P1 = bp.commit(As, Bs)
            P2 = bp.commit(As, Bs, "inner")
            ab1, xs1, lr1, head1, trs1 = bp.prove1_packed(P1, cs, As, Bs, seeds)
            ab2, xs2, lr2, trs2 = bp.prove2_packed(As, Bs)
        finally:
            bp.close()
    assert len(P1) == len(P2) == count and all(a.to_le64() != b.to_le64() for a, b in zip(P1, P2))
    bv = BatchInnerProductVerifier(g, h)
    try:
        assert bv.verify_packed1(u, P1, cs, ab1, xs1, lr1, head1, trs1) is True
        assert bv.verify_packed2([u] * count, P2, ab2, xs2, lr2, trs2) is True
        moved1 = P1[:3] + [P1[3] + secp256k1.G] + P1[4:]
        moved2 = P2[:1] + [P2[1] + secp256k1.G] + P2[2:]
        assert bv.verify_packed1(u, moved1, cs, ab1, xs1, lr1, head1, trs1) is False
        assert bv.verify_packed2([u] * count, moved2, ab2, xs2, lr2, trs2) is False
    finally:
        bv.release()


# ---- 8. the C ABI ------------------------------------------------------------------------------------------------------------
def test_c_abi_refusals(gp):
    """Every refusal of include/bpmi.h returns BPMI_E_ARG with its cause in the message and leaves the output as it was."""
    eng = gp.engine()
    lib = eng.lib
    n, count = 4, 3
    pts = _points(gp, 2 * n + 1, 2800)
    gb, hb, ub = (b"".join(p.to_le64() for p in pts[:n]), b"".join(p.to_le64() for p in pts[n: 2 * n]), pts[2 * n].to_le64())
    As, Bs = _vectors(n, count, 81), _vectors(n, count, 82)
    a, b, t = _sc(v for row in As for v in row), _sc(v for row in Bs for v in row), _sc(random.Random(83).randrange(Q) for _ in range(count))
    fill = bytes([0xAB]) * (64 * count)
    out = ctypes.create_string_buffer(fill, 64 * count)
    vp = lambda x: None if x is None else ctypes.cast(x, ctypes.c_void_p)
    fn = lib.bpmi_ipa_batch_prover_commit_batch

    def err(ctx=eng.ctx):
        return lib.bpmi_last_error(ctx).decode()

    assert fn(None, count, a, b, 0, None, vp(out)) == E_ARG and "bpmi_ipa_batch_prover_commit_batch" in err(None) and "(pv)" in err(None)
    assert out.raw == fill
    handle = ctypes.c_void_p()
    with _Options(eng, prover_table_bits=6):
        eng._ck(lib.bpmi_ipa_batch_prover_create(eng.ctx, n, gb, hb, ub, None, ctypes.byref(handle)))
    pv = handle.value
    try:
        bad_q = Q.to_bytes(32, "little")
        refusals = [
            ((count, a, b, 0, None, None), "null argument (out)"),
            ((count, a, b, -1, None, vp(out)), "u_mode must be 0"), ((count, a, b, 3, None, vp(out)), "u_mode must be 0"),
            ((count, a, b, 0, t, vp(out)), "t must be NULL unless u_mode is 2"), ((count, a, b, 1, t, vp(out)), "t must be NULL unless u_mode is 2"),
            ((count, a, b, 2, None, vp(out)), "u_mode 2 takes t"),
            ((count, None, None, 0, None, vp(out)), "a and b are both NULL"), ((count, None, None, 2, t, vp(out)), "a and b are both NULL"),
            ((count, a, None, 1, None, vp(out)), "it takes both a and b"), ((count, None, b, 1, None, vp(out)), "it takes both a and b"),
            (((1 << 20) + 1, a[:32], b[:32], 0, None, vp(out)), "2^20 proofs"),                       # (nothing of the short arrays is read)
            ((count, a[: 32 * 5] + bad_q + a[32 * 6:], b, 0, None, vp(out)), "a[5] is not below the group order"),
            ((count, a, b[: 32 * 11] + b"\xff" * 32, 1, None, vp(out)), "b[11] is not below the group order"),
            ((count, None, b[: 32 * 2] + bad_q + b[32 * 3:], 0, None, vp(out)), "b[2] is not below the group order"),
            ((count, a, b, 2, t[:32] + bad_q + t[64:], vp(out)), "t[1] is not below the group order"),
            ((0, a, b, 3, None, vp(out)), "u_mode must be 0"),
        ]
        for args, text in refusals:
            assert fn(pv, *args) == E_ARG, args
            assert "bpmi_ipa_batch_prover_commit_batch: " in err() and text in err(), (args, err())
            assert out.raw == fill, args
        assert fn(pv, 0, None, None, 0, None, None) == 0 and fn(pv, 0, a, b, 1, None, vp(out)) == 0
        assert out.raw == fill
        ms = (ctypes.c_double * 2)()
        assert lib.bpmi_ipa_batch_prover_commit_last_ms(pv, None) == E_ARG and lib.bpmi_ipa_batch_prover_commit_last_ms(None, ms) == E_ARG
        # and the same arrays, accepted
        eng._ck(fn(pv, count, a, b, 2, t, vp(out)))
        orc = _Oracle(pts[:n], pts[n: 2 * n], pts[2 * n])
        assert out.raw == orc.many(As, Bs, [int.from_bytes(t[32 * i: 32 * i + 32], "little") for i in range(count)])
        eng._ck(lib.bpmi_ipa_batch_prover_commit_last_ms(pv, ms))
        assert ms[0] > 0 and ms[1] >= ms[0]
    finally:
        lib.bpmi_ipa_batch_prover_destroy(pv)
    # 2^27 elements: a prover of 1 024 elements takes at most 2^17 statements; refused before a read of the (one-scalar) arrays
    n = 1024
    wide = b"".join(p.to_le64() for p in _points(gp, 2 * n + 1, 2801))
    with _Options(eng, prover_table_bits=6):
        eng._ck(lib.bpmi_ipa_batch_prover_create(eng.ctx, n, wide[: 64 * n], wide[64 * n: 128 * n], wide[128 * n:], None, ctypes.byref(handle)))
    try:
        one = ctypes.create_string_buffer(bytes([0xCD]) * 64, 64)
        assert fn(handle.value, (1 << 17) + 1, bytes(32), bytes(32), 0, None, vp(one)) == E_ARG and "2^27 elements" in err()
        assert fn(handle.value, (1 << 17) + 1, bytes(32), bytes(32), 2, bytes(32), vp(one)) == E_ARG and "2^27 elements" in err()
        assert fn(handle.value, (1 << 20) + 1, bytes(32), None, 0, None, vp(one)) == E_ARG and "2^20 proofs" in err()
        assert one.raw == bytes([0xCD]) * 64
    finally:
        lib.bpmi_ipa_batch_prover_destroy(handle.value)
