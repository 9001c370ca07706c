"""GPU parity of the batched inner-product prover (bpmi_ipa_prove_batch, innerproduct/batch_prover.py): every proof of a batch is
identical, field for field, to the one the single-proof provers of the same build make for the same inputs -- NIProver.prove
(src/innerproduct/inner_product_prover.py:11-45) and FastNIProver2.prove (:48-110), themselves pinned to the
reference's goldens by tests/test_gpu_ipa.py -- and to the goldens directly (tests/golden/ipa.json); the proofs pass the batch
verifier, and the C ABI refuses what include/bpmi.h says it refuses.

Unless a test says otherwise the tables are built with 6-bit windows (180 MB at n = 1 024); every prover is closed in `finally`.

The issue's case "a = 0: every L and R is the identity" holds only when b is zero too (L = <a_lo, g_hi> + <b_hi, h_lo> + c_L u): here
a = 0 and b = 0 are compared with the single-proof prover each, and a = b = 0 carries the identity / "AA==" assertions."""
import ctypes
import random
from base64 import b64encode

import pytest

from conftest import load_golden
from helpers import P as OP, Q, gens, hx, scal
from oracle import bp_ref as R

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
    from bulletproofs_amd.utils import ModP
    rnd = random.Random(seed)
    return [[ModP(rnd.randrange(Q), Q) for _ in range(n)] for _ in range(count)]


def _seeds(count, rnd):
    lens = (0, 1, 2, 3, 17, 200)
    return [rnd.randbytes(lens[i % len(lens)]) for i in range(count)]


def _prefixes(count):
    kinds = (b"", b"one&", b"1&22&333&", None, b"raw")
    return [kinds[i % len(kinds)] for i in range(count)]


def f2(p):
    return (p.a.x, p.b.x, [x.x for x in p.xs], [pt.to_le64() for pt in p.Ls], [pt.to_le64() for pt in p.Rs], p.transcript, p.start_transcript)


def f1(p):
    return (p.u_new.to_le64(), p.P_new.to_le64(), p.transcript) + f2(p.proof2)


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


def _check_against_single(gp, g, h, u, Ps, cs, As, Bs, seeds, prefixes, h_scale=None, bp=None):
    """Both protocols of one prover against NIProver / FastNIProver2, every field of every proof."""
    from bulletproofs_amd.ec import secp256k1
    from bulletproofs_amd.innerproduct import BatchInnerProductProver, FastNIProver2, NIProver
    own = bp is None
    if own:
        bp = BatchInnerProductProver(g, h, u, h_scale=h_scale)
    try:
        got1 = bp.prove1(Ps, cs, As, Bs, seeds)
        got2 = bp.prove2(As, Bs, prefixes)
    finally:
        if own:
            bp.close()
    assert len(got1) == len(got2) == len(As)
    for i in range(len(As)):
        want1 = NIProver(g, h, u, Ps[i], cs[i], As[i], Bs[i], secp256k1, seeds[i], h_scale=h_scale).prove()
        assert f1(got1[i]) == f1(want1), ("protocol 1", i)
        want2 = FastNIProver2(g, h, u, Ps[i], As[i], Bs[i], secp256k1, prefixes[i], h_scale=h_scale).prove()
        assert f2(got2[i]) == f2(want2), ("protocol 2", i)
    return got1, got2


def _inner(a, b):
    from bulletproofs_amd.utils import ModP
    return ModP(sum(x.x * y.x for x, y in zip(a, b)) % Q, Q)


# ---- 1. shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,count,table_bits,job_lanes", [(1, 5, 6, 0), (2, 70, 6, 0), (4, 130, 6, 0), (64, 70, 6, 0), (256, 3, 6, 0), (512, 2, 6, 0),
                                                          (1024, 2, 6, 0), (256, 3, 6, 16), (256, 3, 6, 64), (4, 9, 0, 0), (8, 9, 13, 0)])
def test_batch_equals_the_single_proof_provers(gp, n, count, table_bits, job_lanes):
    """Zero rounds, many proofs per wave, a partial last block, one proof per block, the NT = 512 / 1 024 instantiations, both job
    widths, the default 16-bit tables (302 MB at n = 4) and 13-bit ones (20 windows, the top one short)."""
    pts = _points(gp, 2 * n + 1 + count, 100 + n)
    g, h, u, Ps = pts[:n], pts[n: 2 * n], pts[2 * n], pts[2 * n + 1:]
    As, Bs = _vectors(n, count, 7 * n + count), _vectors(n, count, 11 * n + count)
    cs = [_inner(a, b) for a, b in zip(As, Bs)]
    rnd = random.Random(n + count)
    with _Options(gp.engine(), prover_table_bits=table_bits, prover_job_lanes=job_lanes):
        _check_against_single(gp, g, h, u, Ps, cs, As, Bs, _seeds(count, rnd), _prefixes(count))


def test_c_null_is_the_inner_product(gp):
    """c = NULL: c_p = <a_p, b_p>, summed on the device (n = 1: a single product; n = 16; n = 512: a tree over a whole block)."""
    from bulletproofs_amd.innerproduct import BatchInnerProductProver
    for n, count in ((1, 3), (16, 20), (512, 2)):
        pts = _points(gp, 2 * n + 1 + count, 300 + n)
        g, h, u, Ps = pts[:n], pts[n: 2 * n], pts[2 * n], pts[2 * n + 1:]
        As, Bs = _vectors(n, count, n), _vectors(n, count, n + 1)
        seeds = _seeds(count, random.Random(n))
        with _Options(gp.engine(), prover_table_bits=6):
            bp = BatchInnerProductProver(g, h, u)
            try:
                given = bp.prove1(Ps, [_inner(a, b) for a, b in zip(As, Bs)], As, Bs, seeds)
                summed = bp.prove1(Ps, None, As, Bs, seeds)
            finally:
                bp.close()
        assert [f1(p) for p in summed] == [f1(p) for p in given]


# ---- 2. goldens --------------------------------------------------------------------------------------------------------------
def _check_golden2(gp, p2, want):
    assert hx(p2.a.x) == want["a"] and hx(p2.b.x) == want["b"]
    assert [hx(x.x) for x in p2.xs] == want["xs"]
    assert len(p2.Ls) == len(want["Ls"]) and all(gp.same_point(a, OP(b)) for a, b in zip(p2.Ls, want["Ls"]))
    assert len(p2.Rs) == len(want["Rs"]) and all(gp.same_point(a, OP(b)) for a, b in zip(p2.Rs, want["Rs"]))
    assert p2.transcript.decode() == want["transcript"]
    assert p2.start_transcript == want["start_transcript"]


@pytest.mark.parametrize("k", range(9))
def test_reference_goldens(gp, k):
    """The cases n = 1 .. 256 of tests/golden/ipa.json rebuilt from their seeds; one prover per n, a batch of 3 copies."""
    from bulletproofs_amd.innerproduct import BatchInnerProductProver
    c = load_golden("ipa.json")["cases"][k]
    n = c["n"]
    s = [bytes.fromhex(x) for x in c["seeds"]]
    g, h, u = gp.to_gpu_list(gens(n, s[0])), gp.to_gpu_list(gens(n, s[1])), gp.to_gpu(R.elliptic_hash(s[2]))
    a, b = [gp.gsc(v) for v in scal(n, s[3])], [gp.gsc(v) for v in scal(n, s[4])]
    ip = _inner(a, b)
    assert hx(ip.x) == c["c"]
    P1 = gp.to_gpu(OP(c["P1"]))
    with _Options(gp.engine(), prover_table_bits=6):
        bp = BatchInnerProductProver(g, h, u)
        try:
            got2 = bp.prove2([a] * 3, [b] * 3)
            got1 = bp.prove1([P1] * 3, [ip] * 3, [a] * 3, [b] * 3, [s[5]] * 3)
        finally:
            bp.close()
    for p2 in got2:
        _check_golden2(gp, p2, c["proof2"])
    for p1 in got1:
        assert gp.same_point(p1.u_new, OP(c["proof1"]["u_new"])) and gp.same_point(p1.P_new, OP(c["proof1"]["P_new"]))
        assert p1.transcript.decode() == c["proof1"]["transcript"]
        _check_golden2(gp, p1.proof2, c["proof1"]["proof2"])


# ---- 3. scalars at the edges -------------------------------------------------------------------------------------------------
def test_scalars_at_the_edges(gp):
    from bulletproofs_amd.ec import Point
    from bulletproofs_amd.utils import ModP
    n = 8
    pts = _points(gp, 2 * n + 1 + 6, 808)
    g, h, u, Ps = pts[:n], pts[n: 2 * n], pts[2 * n], pts[2 * n + 1:]
    ra, rb = _vectors(n, 1, 1)[0], _vectors(n, 1, 2)[0]
    zero, top = [ModP(0, Q)] * n, [ModP(Q - 1, Q)] * n
    low = ra[: n // 2] + zero[: n // 2]
    high = zero[: n // 2] + ra[n // 2:]
    As = [zero, ra, top, low, high, zero]
    Bs = [rb, zero, top, rb, rb, zero]
    cs = [_inner(a, b) for a, b in zip(As, Bs)]
    rnd = random.Random(3)
    with _Options(gp.engine(), prover_table_bits=6):
        got1, got2 = _check_against_single(gp, g, h, u, Ps, cs, As, Bs, _seeds(6, rnd), _prefixes(6))
    ident = Point.IDENTITY_ELEMENT.to_le64()
    assert ident == bytes(64)
    for p2 in (got1[5].proof2, got2[5]):                   # a = b = 0: every L and R is the identity
        assert [pt.to_le64() for pt in p2.Ls + p2.Rs] == [ident] * 6
        assert p2.transcript.count(b"AA==&") == 6 and (p2.a.x, p2.b.x) == (0, 0)
    assert got2[0].a.x == 0 and got2[1].b.x == 0


def test_wrong_c_is_proved_as_given_and_rejected(gp):
    from bulletproofs_amd.ec import secp256k1
    from bulletproofs_amd.innerproduct import BatchInnerProductProver, NIProver, Verifier1
    from bulletproofs_amd.utils import ModP, vector_commitment
    n = 8
    pts = _points(gp, 2 * n + 1, 909)
    g, h, u = pts[:n], pts[n: 2 * n], pts[2 * n]
    a, b = _vectors(n, 1, 5)[0], _vectors(n, 1, 6)[0]
    P1 = vector_commitment(g, h, a, b)
    good, bad = _inner(a, b), _inner(a, b) + ModP(1, Q)
    with _Options(gp.engine(), prover_table_bits=6):
        bp = BatchInnerProductProver(g, h, u)
        try:
            got = bp.prove1([P1, P1], [good, bad], [a, a], [b, b], [b"s", b"s"])
        finally:
            bp.close()
    assert f1(got[1]) == f1(NIProver(g, h, u, P1, bad, a, b, secp256k1, b"s").prove())
    assert Verifier1(g, h, u, P1, good, got[0]).verify() is True
    with pytest.raises(Exception, match="Proof invalid"):
        Verifier1(g, h, u, P1, bad, got[1]).verify()


def test_h_scale_with_zero_one_and_q_minus_one(gp):
    n = 8
    pts = _points(gp, 2 * n + 1 + 4, 1010)
    g, h, u, Ps = pts[:n], pts[n: 2 * n], pts[2 * n], pts[2 * n + 1:]
    rnd = random.Random(10)
    scale = [0, 1, Q - 1] + [rnd.randrange(1, Q) for _ in range(n - 3)]
    As, Bs = _vectors(n, 4, 12), _vectors(n, 4, 13)
    cs = [_inner(a, b) for a, b in zip(As, Bs)]
    with _Options(gp.engine(), prover_table_bits=6):
        _check_against_single(gp, g, h, u, Ps, cs, As, Bs, _seeds(4, rnd), _prefixes(4), h_scale=scale)


# ---- 4. generators at the edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,variant", [(4, "collide"), (8, "collide"), (4, "h_is_g"), (8, "h_is_g")])
def test_generators_at_the_edges(gp, n, variant):
    """g_1 = g_0, h_0 = -g_0, g_2 = the identity; and h = g: table rows that coincide, cancel or are empty."""
    from bulletproofs_amd.ec import Point
    pts = _points(gp, 2 * n + 1 + 5, 1100 + n)
    g, h, u, Ps = pts[:n], pts[n: 2 * n], pts[2 * n], pts[2 * n + 1:]
    if variant == "collide":
        g[1] = g[0]
        h[0] = -g[0]
        g[2] = Point.IDENTITY_ELEMENT
    else:
        h = list(g)
    As, Bs = _vectors(n, 5, n), _vectors(n, 5, n + 50)
    As[1] = [As[1][0]] * n                                  # equal scalars on the coinciding generators: lanes' partial sums that coincide
    cs = [_inner(a, b) for a, b in zip(As, Bs)]
    with _Options(gp.engine(), prover_table_bits=6):
        _check_against_single(gp, g, h, u, Ps, cs, As, Bs, _seeds(5, random.Random(n)), _prefixes(5))


# ---- 5. the head -------------------------------------------------------------------------------------------------------------
def test_the_head_at_the_identity_and_the_doubling(gp):
    """P = the identity; P = -(x c) u, so P_new is the identity; P = (x c) u, so the addition is a doubling.  x = mod_hash(base64(seed) "&")."""
    from bulletproofs_amd.ec import Point
    from bulletproofs_amd.pippenger import PipSECP256k1
    from bulletproofs_amd.utils.utils import mod_hash
    n = 4
    pts = _points(gp, 2 * n + 1, 1200)
    g, h, u = pts[:n], pts[n: 2 * n], pts[2 * n]
    As, Bs = _vectors(n, 3, 21), _vectors(n, 3, 22)
    cs = [_inner(a, b) for a, b in zip(As, Bs)]
    seeds = [b"", b"head", b"double!"]
    xcu = [PipSECP256k1.multiexp([u], [mod_hash(b64encode(sd) + b"&", Q).x * c.x % Q]) for sd, c in zip(seeds, cs)]
    Ps = [Point.IDENTITY_ELEMENT, -xcu[1], xcu[2]]
    with _Options(gp.engine(), prover_table_bits=6):
        got1, _ = _check_against_single(gp, g, h, u, Ps, cs, As, Bs, seeds, _prefixes(3))
    assert got1[0].P_new.to_le64() == xcu[0].to_le64()
    assert got1[1].P_new.to_le64() == bytes(64)
    assert got1[2].P_new.to_le64() == PipSECP256k1.multiexp([xcu[2]], [2]).to_le64()


# ---- 6. seeds ----------------------------------------------------------------------------------------------------------------
def test_seeds_of_every_padding_and_prefixes(gp):
    """Seeds of 0, 1, 2, 3 and 200 bytes (every base64 padding) and prefixes of 0, 1 and 3 '&'-separated items, in ONE batch each."""
    n = 16
    pts = _points(gp, 2 * n + 1 + 5, 1300)
    g, h, u, Ps = pts[:n], pts[n: 2 * n], pts[2 * n], pts[2 * n + 1:]
    As, Bs = _vectors(n, 5, 31), _vectors(n, 5, 32)
    cs = [_inner(a, b) for a, b in zip(As, Bs)]
    rnd = random.Random(6)
    seeds = [b"", b"\xfb", b"\xff\xfe", b"abc", rnd.randbytes(200)]
    prefixes = [b"", b"one&", b"1&22&333&", None, b"x" * 200 + b"&"]
    with _Options(gp.engine(), prover_table_bits=6):
        got1, got2 = _check_against_single(gp, g, h, u, Ps, cs, As, Bs, seeds, prefixes)
    assert [p.start_transcript for p in got2] == [1, 2, 4, 1, 2]
    assert [p.transcript.split(b"&")[0] for p in got1] == [b64encode(s) for s in seeds]


# ---- 7. state ----------------------------------------------------------------------------------------------------------------
def test_a_prover_is_reusable(gp):
    """A second, smaller batch on the same prover equals the prefix of the first; a Protocol-2 call after a Protocol-1 call (and back) is right."""
    from bulletproofs_amd.innerproduct import BatchInnerProductProver
    n, count = 16, 23
    pts = _points(gp, 2 * n + 1 + count, 1400)
    g, h, u, Ps = pts[:n], pts[n: 2 * n], pts[2 * n], pts[2 * n + 1:]
    As, Bs = _vectors(n, count, 41), _vectors(n, count, 42)
    seeds = _seeds(count, random.Random(7))
    with _Options(gp.engine(), prover_table_bits=6):
        bp = BatchInnerProductProver(g, h, u)
        try:
            first = bp.prove1_packed(Ps, None, As, Bs, seeds)
            second = bp.prove1_packed(Ps[:5], None, As[:5], Bs[:5], seeds[:5])
            p2 = bp.prove2_packed(As, Bs)
            third = bp.prove1_packed(Ps[:5], None, As[:5], Bs[:5], seeds[:5])
            p2_small = bp.prove2_packed(As[:7], Bs[:7])
        finally:
            bp.close()
    k = 4
    for sizes, whole, part, m in (((64, 32 * k, 128 * k, 128), first, second, 5), ((64, 32 * k, 128 * k), p2, p2_small, 7)):
        for size, w, s in zip(sizes, whole, part):
            assert s == w[: size * m]
        assert part[-1] == whole[-1][:m]
    assert third == second


# ---- 8. round trip -----------------------------------------------------------------------------------------------------------
def test_round_trip_through_the_batch_verifier(gp):
    from bulletproofs_amd.innerproduct import BatchInnerProductProver, BatchInnerProductVerifier
    from bulletproofs_amd.utils import ModP, vector_commitment_batch
    n, count = 16, 40
    pts = _points(gp, 2 * n + 1, 1500)
    g, h, u = pts[:n], pts[n: 2 * n], pts[2 * n]
    As, Bs = _vectors(n, count, 51), _vectors(n, count, 52)
    with _Options(gp.engine(), prover_table_bits=6):
        bp = BatchInnerProductProver(g, h, u)
        try:
            proofs = bp.prove2(As, Bs)
        finally:
            bp.close()
    Ps = [vc + _inner(a, b) * u for vc, a, b in zip(vector_commitment_batch(g, h, As, Bs), As, Bs)]
    bv = BatchInnerProductVerifier(g, h)
    try:
        for P, pr in zip(Ps, proofs):
            bv.add(u, P, pr)
        assert bv.verify() is True and bv.locate() == []
        bv.reset()
        proofs[17].a = proofs[17].a + ModP(1, Q)
        for P, pr in zip(Ps, proofs):
            bv.add(u, P, pr)
        assert bv.verify() is False and bv.locate() == [17]
    finally:
        bv.release()


# ---- 9. the C ABI ------------------------------------------------------------------------------------------------------------
def test_c_abi_refusals(gp):
    """Every refusal of include/bpmi.h returns BPMI_E_ARG with the bound or the index in the message, and leaves the outputs as they were."""
    from bulletproofs_amd.ec import secp256k1
    eng = gp.engine()
    lib = eng.lib
    n, k, count = 4, 2, 3
    pts = _points(gp, 2 * n + 1 + count, 1600)
    gb, hb, ub = (b"".join(p.to_le64() for p in pts[:n]), b"".join(p.to_le64() for p in pts[n: 2 * n]), pts[2 * n].to_le64())
    Pb = b"".join(p.to_le64() for p in pts[2 * n + 1:])
    rnd = random.Random(16)
    sc = lambda m: b"".join(rnd.randrange(Q).to_bytes(32, "little") for _ in range(m))
    a, b, c = sc(count * n), sc(count * n), sc(count)

    def err():
        return lib.bpmi_last_error(eng.ctx).decode()

    handle = ctypes.c_void_p()
    for bad_n in (0, 3, 2048):
        assert lib.bpmi_ipa_batch_prover_create(eng.ctx, bad_n, gb, hb, ub, None, ctypes.byref(handle)) == E_ARG and handle.value is None
        assert "power of two" in err() and "1024" in err()
    assert lib.bpmi_ipa_batch_prover_create(eng.ctx, n, gb, bytes(64) + b"\x01" + bytes(63) + hb[128:], ub, None, ctypes.byref(handle)) == E_ARG
    assert "h[1] is not a point of the curve" in err() and handle.value is None
    assert lib.bpmi_ipa_batch_prover_create(eng.ctx, n, gb, hb, ub, bytes(32) + b"\xff" * 32 + bytes(64), ctypes.byref(handle)) == E_ARG
    assert "h_scale[1]" in err() and handle.value is None
    eng.set_option("prover_table_bits", 6)
    try:
        eng._ck(lib.bpmi_ipa_batch_prover_create(eng.ctx, n, gb, hb, ub, None, ctypes.byref(handle)))
    finally:
        eng.set_option("prover_table_bits", 0)
    pv = handle.value
    try:
        need = lib.bpmi_ipa_prove_batch_transcript_bytes(pv, 1, 3)
        assert need == 1 + 4 + 1 + 79 + k * (45 + 45 + 79) and lib.bpmi_ipa_prove_batch_transcript_bytes(pv, 2, 3) == 1 + 3 + k * 169
        assert lib.bpmi_ipa_prove_batch_transcript_bytes(pv, 3, 0) == 0
        cap = count * need
        fill = 0xAB
        outs = dict(ab=ctypes.create_string_buffer(bytes([fill]) * (64 * count), 64 * count), xs=ctypes.create_string_buffer(bytes([fill]) * (32 * k * count), 32 * k * count),
                    LR=ctypes.create_string_buffer(bytes([fill]) * (128 * k * count), 128 * k * count), head=ctypes.create_string_buffer(bytes([fill]) * (128 * count), 128 * count),
                    tr=ctypes.create_string_buffer(bytes([fill]) * cap, cap))
        tr_off = (ctypes.c_uint64 * (count + 1))(*([7] * (count + 1)))
        seeds, off = b"abcdefgh", (ctypes.c_uint64 * (count + 1))(0, 3, 5, 8)
        vp = lambda x: None if x is None else ctypes.cast(x, ctypes.c_void_p)

        def call(protocol=1, n_proofs=count, a_=a, b_=b, c_=c, P_=Pb, seeds_=seeds, off_=off, cap_=cap, **drop):
            assert set(drop) <= set(outs) | {"tr_off"}                   # an output named here is handed in as NULL
            o = {name: (None if name in drop else buf) for name, buf in outs.items()}
            return lib.bpmi_ipa_prove_batch(pv, protocol, n_proofs, a_, b_, c_, P_, seeds_, off_, vp(o["ab"]), vp(o["xs"]), vp(o["LR"]), vp(o["head"]), vp(o["tr"]), cap_,
                                            None if "tr_off" in drop else tr_off)

        def untouched():
            return all(buf.raw == bytes([fill]) * len(buf.raw) for buf in outs.values()) and list(tr_off) == [7] * (count + 1)

        refusals = [
            (dict(protocol=0), "protocol must be 1 or 2"), (dict(protocol=3), "protocol must be 1 or 2"),
            (dict(a_=None), "null argument"), (dict(b_=None), "null argument"), (dict(P_=None), "null argument"), (dict(off_=None), "null argument"),
            (dict(ab=None), "null argument"), (dict(xs=None), "null argument"), (dict(LR=None), "null argument"), (dict(head=None), "null argument"),
            (dict(tr=None), "null argument"), (dict(tr_off=None), "null argument"),
            (dict(protocol=2, c_=None, P_=None), "must be NULL under Protocol 2"),                       # head non-NULL
            (dict(protocol=2, P_=None, head=None), "must be NULL under Protocol 2"),                      # c non-NULL
            (dict(protocol=2, c_=None, head=None), "must be NULL under Protocol 2"),                      # P non-NULL
            (dict(n_proofs=(1 << 20) + 1, cap_=0, a_=a[:32], b_=b[:32]), "2^20 proofs"),                  # (nothing of the short arrays is read)
            (dict(off_=(ctypes.c_uint64 * 4)(0, 65536, 65536, 65536), seeds_=bytes(65536)), "65535"),
            (dict(off_=(ctypes.c_uint64 * 4)(0, 5, 3, 8)), "must not decrease"),
            (dict(seeds_=None), "null argument"),
            (dict(cap_=cap - 1), "too small"), (dict(cap_=0), "too small"),
            (dict(a_=a[: 32 * 5] + Q.to_bytes(32, "little") + a[32 * 6:]), "a[5] is not below the group order"),
            (dict(b_=b[: 32 * 11] + b"\xff" * 32), "b[11] is not below the group order"),
            (dict(c_=c[:32] + Q.to_bytes(32, "little") + c[64:]), "c[1] is not below the group order"),
            (dict(P_=Pb[:128] + (1).to_bytes(32, "little") + (1).to_bytes(32, "little")), "P[2] is not a point of the curve"),
            (dict(P_=Pb[:64] + secp256k1.p.to_bytes(32, "little") + bytes(32) + Pb[128:]), "P[1] is not a point of the curve"),
        ]
        for kwargs, text in refusals:
            assert call(**kwargs) == E_ARG, kwargs
            assert text in err(), (kwargs, err())
            assert untouched(), kwargs
        assert lib.bpmi_ipa_prove_batch(pv, 1, 0, None, None, None, None, None, None, None, None, None, None, None, 0, None) == 0
        assert lib.bpmi_ipa_prove_batch(pv, 2, 0, None, None, None, None, None, None, None, None, None, None, None, 0, None) == 0
        assert untouched()
        ms = (ctypes.c_double * 4)()
        assert lib.bpmi_ipa_batch_prover_last_ms(pv, None) == E_ARG and lib.bpmi_ipa_batch_prover_last_ms(None, ms) == E_ARG
        # and the same arrays, accepted: with c NULL and seeds of 3, 2 and 3 bytes
        eng._ck(call(c_=None))
        assert not untouched() and list(tr_off)[0] == 0 and tr_off[count] <= cap
        assert outs["tr"].raw[: tr_off[1]].startswith(b"&" + b64encode(b"abc") + b"&")
        eng._ck(lib.bpmi_ipa_batch_prover_last_ms(pv, ms))
        assert ms[3] > 0 and abs(ms[0] + ms[1] + ms[2] - ms[3]) < 0.05 * ms[3] + 0.01
    finally:
        lib.bpmi_ipa_batch_prover_destroy(pv)
    lib.bpmi_ipa_batch_prover_destroy(None)
    # 2^27 elements: a prover of 1 024 elements takes at most 2^17 proofs, fewer than the 2^20 of the other cap
    n = 1024
    wide = b"".join(p.to_le64() for p in _points(gp, 2 * n + 1, 1601))
    eng.set_option("prover_table_bits", 6)
    try:
        eng._ck(lib.bpmi_ipa_batch_prover_create(eng.ctx, n, wide[: 64 * n], wide[64 * n: 128 * n], wide[128 * n:], None, ctypes.byref(handle)))
    finally:
        eng.set_option("prover_table_bits", 0)
    try:
        one = ctypes.create_string_buffer(64)
        args = (bytes(32), bytes(32), None, None, None, (ctypes.c_uint64 * 1)(0), vp(one), vp(one), vp(one), None, vp(one), 0, (ctypes.c_uint64 * 1)(0))
        assert lib.bpmi_ipa_prove_batch(handle.value, 2, (1 << 17) + 1, *args) == E_ARG and "2^27 elements" in err()
        assert lib.bpmi_ipa_prove_batch(handle.value, 2, (1 << 20) + 1, *args) == E_ARG and "2^20 proofs" in err()
        assert one.raw == bytes(64)
    finally:
        lib.bpmi_ipa_batch_prover_destroy(handle.value)
