"""GPU tests of the batch verifier of inner-product proofs: the weighted s-vector sums (bpmi_sc_svector_sum) against Python integers,
BatchInnerProductVerifier end to end against Verifier2 / Verifier1 proof by proof, the random weights, and the argument errors of
bpmi_ipa_verify_batch_dev.  The Protocol-1 cheating cases are those of /root/reference/src/tests/test_innerprod.py that
tests/test_gpu_ipa.py mirrors per proof."""
import copy
import ctypes
import functools
import random

import pytest

from conftest import load_golden
from helpers import P as GoldenPoint
from helpers import Q, gens, scal
from ipa_batch_ref import draw_proofs, draw_scale, ref_sums
from oracle import bp_ref as R
from oracle import cbind

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gp():
    import gpu_common
    return gpu_common


def pack(vals):
    return b"".join((v % Q).to_bytes(32, "little") for v in vals)


def unpack(raw):
    return [int.from_bytes(raw[i: i + 32], "little") for i in range(0, len(raw), 32)]


# ---- bpmi_sc_svector_sum ----------------------------------------------------------------------------------------------------------
# n = 1; kl = 0; odd k; n below a wave; a table half of exactly 64 records (k = 13: kl = 6); one proof; a last range shorter than the
# others (65 and 130 proofs); many proofs against few elements (parts > 1)
SUM_SHAPES = [(0, 1), (0, 3), (1, 2), (2, 1), (3, 5), (5, 64), (6, 65), (7, 3), (11, 2), (13, 130)]


@functools.lru_cache(maxsize=None)
def sum_case(k, proofs):
    ps = draw_proofs(k, proofs, 31 * k + proofs)
    scale = draw_scale(k, 5 + k)
    return ps, scale, ref_sums(k, ps)


def sum_call(eng, k, ps, scale=None):
    sa, sb = eng.sc_svector_sum_bytes(k, len(ps), pack([x for p in ps for x in p[0]]), pack([pow(x, -1, Q) for p in ps for x in p[0]]),
                                      pack([p[1] for p in ps]), pack([p[2] for p in ps]), pack([p[3] for p in ps]),
                                      None if scale is None else pack(scale))
    return unpack(sa), unpack(sb)


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scale"])
@pytest.mark.parametrize("k,proofs", SUM_SHAPES)
def test_svector_sum_equals_python_integers(gp, k, proofs, scaled):
    ps, scale, (sa, sb) = sum_case(k, proofs)
    assert any(p[1] == 0 for p in ps) and (proofs < 2 or any(p[2] == 0 for p in ps))           # a = 0 and b = 0 are among the proofs
    got_a, got_b = sum_call(gp.engine(), k, ps, scale if scaled else None)
    assert got_a == sa
    assert got_b == ([v * c % Q for v, c in zip(sb, scale)] if scaled else sb)


@pytest.mark.parametrize("k,proofs", [(0, 3), (3, 5), (7, 3), (12, 4), (6, 65)])
def test_svector_sum_with_unit_weights_is_the_sum_of_single_svectors(gp, k, proofs):
    """w = 1 for every proof: the sum of `proofs` calls of the existing bpmi_sc_svector (k = 12: both table halves are 64 records)."""
    eng = gp.engine()
    ps = [(xs, a, b, 1) for xs, a, b, _ in draw_proofs(k, proofs, 900 + k)]
    scale = draw_scale(k, 3)
    for sc in (None, scale):
        want_a, want_b = [0] * (1 << k), [0] * (1 << k)
        for xs, a, b, _ in ps:
            ra, rb = eng.sc_svector_bytes(pack(xs), pack([pow(x, -1, Q) for x in xs]), k, a, b, None if sc is None else pack(sc))
            want_a = [(v + t) % Q for v, t in zip(want_a, unpack(ra))]
            want_b = [(v + t) % Q for v, t in zip(want_b, unpack(rb))]
        assert sum_call(eng, k, ps, sc) == (want_a, want_b)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
class Statement:
    def __init__(self, u, P, proof):
        self.u, self.P, self.proof = u, P, proof


def single_verdict(g, h, st, scale):
    from bulletproofs_amd.innerproduct import Verifier2
    try:
        return Verifier2(g, h, st.u, st.P, st.proof, scale).verify() is True
    except Exception as e:
        assert "Proof invalid" in str(e)
        return False


def prove_statements(gp, g, h, n, count, scale, seed, same_u=False):
    from bulletproofs_amd.ec import secp256k1
    from bulletproofs_amd.innerproduct import FastNIProver2
    from bulletproofs_amd.utils import ModP, inner_product, vector_commitment
    rnd = random.Random(seed)
    us = gp.to_gpu_list(gp.rand_points(count, seed + 1)[0])
    out = []
    for p in range(count):
        u = us[0] if same_u else us[p]
        a = [ModP(rnd.randrange(Q), Q) for _ in range(n)]
        b = [ModP(rnd.randrange(Q), Q) for _ in range(n)]
        bs = b if scale is None else [v * c for v, c in zip(b, scale)]
        Pt = vector_commitment(g, h, a, bs) + inner_product(a, b) * u
        out.append(Statement(u, Pt, FastNIProver2(g, h, u, Pt, a, b, secp256k1, h_scale=scale).prove()))
    return out


@pytest.fixture(scope="module")
def generators(gp):
    from bulletproofs_amd.ec import PackedPoints
    pts = gp.to_gpu_list(gp.rand_points(4096, 4242)[0])
    return {n: (PackedPoints(pts[:n]), PackedPoints(pts[2048: 2048 + n])) for n in (1024, 2048)}


@pytest.fixture(scope="module")
def batches(gp, generators):
    """(n, scaled) -> generators, scale and five valid statements with distinct (a, b) and distinct u, proved once."""
    made = {}

    def get(n, scaled):
        if (n, scaled) not in made:
            g, h = generators[n]
            scale = [random.Random(n).randrange(1, Q) for _ in range(n)] if scaled else None
            made[(n, scaled)] = (g, h, scale, prove_statements(gp, g, h, n, 5, scale, 10 * n + scaled))
        return made[(n, scaled)]
    return get


def make_verifier(gp, g, h, scale, sts, counter=None):
    from bulletproofs_amd.innerproduct import BatchInnerProductVerifier
    eng = gp.engine()
    bv = BatchInnerProductVerifier(g, h, scale, engine=eng)
    if counter is not None:
        inner = eng.ipa_verify_batch_dev

        class Counting:
            def __getattr__(self, name):
                return getattr(eng, name)

            def ipa_verify_batch_dev(self, *a, **kw):
                counter.append(a[3])                      # n_proofs of the call
                return inner(*a, **kw)
        bv.engine = Counting()
    assert [bv.add(s.u, s.P, s.proof) for s in sts] == list(range(len(sts)))
    return bv


@pytest.mark.parametrize("n,scaled", [(1024, False), (1024, True), (2048, False), (2048, True)])
def test_batch_accepts_valid_proofs_and_names_a_mutated_one(gp, batches, n, scaled):
    from bulletproofs_amd.innerproduct import batch_verify_inner_products
    from bulletproofs_amd.utils import ModP
    g, h, scale, sts = batches(n, scaled)
    assert all(single_verdict(g, h, s, scale) for s in sts)
    calls = []
    bv = make_verifier(gp, g, h, scale, sts, calls)
    assert bv.verify() is True and calls == [5]
    assert bv.locate() == []
    bv.release()
    assert batch_verify_inner_products(g, h, [(s.u, s.P, s.proof) for s in sts], h_scale=scale, engine=gp.engine()) is True

    def mutate(kind, s):
        m = Statement(s.u, s.P, copy.copy(s.proof))
        if kind == "b+1":
            m.proof.b = s.proof.b + ModP(1, Q)
        elif kind == "P+u":
            m.P = s.P + s.u
        elif kind == "2u":
            m.u = 2 * s.u
        elif kind == "L":
            m.proof.Ls = list(s.proof.Ls)
            m.proof.Ls[1] = s.proof.Rs[2]
        elif kind == "transcript":
            t = bytearray(s.proof.transcript)
            t[len(t) // 2] ^= 1
            m.proof.transcript = bytes(t)
        return m

    for at, kind in enumerate(["b+1", "P+u", "2u", "L", "transcript"]):
        mixed = list(sts)
        mixed[at] = mutate(kind, sts[at])
        assert single_verdict(g, h, mixed[at], scale) is False
        calls = []
        bv = make_verifier(gp, g, h, scale, mixed, calls)
        assert bv.verify() is False
        if kind in ("L", "transcript"):
            assert calls == []                            # the transcript no longer matches: caught on the host, nothing reaches the device
        assert bv.locate() == [at]
        if kind in ("L", "transcript"):
            assert calls and max(calls) <= 4              # the probes run over the four proofs that passed the host checks
        bv.release()


def test_two_invalid_proofs_are_both_named(gp, batches):
    from bulletproofs_amd.utils import ModP
    g, h, scale, sts = batches(1024, False)
    mixed = list(sts)
    for at in (1, 4):
        mixed[at] = Statement(sts[at].u, sts[at].P, copy.copy(sts[at].proof))
        mixed[at].proof.a = sts[at].proof.a + ModP(1, Q)
    bv = make_verifier(gp, g, h, scale, mixed)
    assert bv.verify() is False and bv.locate() == [1, 4]
    bv.reset()
    assert len(bv) == 0 and bv.verify() is True and bv.locate() == []           # an empty batch
    assert bv.add(sts[0].u, sts[0].P, sts[0].proof) == 0 and bv.verify() is True
    bv.release()


def test_the_weights_are_really_used(gp, generators):
    """Two invalid proofs whose errors are -u and +u: they cancel under the weights [1, 1] -- the reason the weights must be random --
    and under no others."""
    g, h = generators[1024]
    s1, s2 = prove_statements(gp, g, h, 1024, 2, None, 99, same_u=True)
    assert s1.u == s2.u
    bad = [Statement(s1.u, s1.P + s1.u, s1.proof), Statement(s2.u, s2.P - s2.u, s2.proof)]
    assert not single_verdict(g, h, bad[0], None) and not single_verdict(g, h, bad[1], None)
    bv = make_verifier(gp, g, h, None, bad)
    assert bv.verify(weights=[1, 1]) is True
    assert bv.verify(weights=[1, 2]) is False
    assert bv.verify(weights=[Q - 1, Q - 1]) is True
    assert bv.verify() is False
    assert bv.locate() == [0, 1]
    with pytest.raises(ValueError):
        bv.verify(weights=[1])
    bv.release()
    good = make_verifier(gp, g, h, None, [s1, s2])
    assert good.verify(weights=[1, 1]) is True and good.verify(weights=[1, 2]) is True and good.verify() is True
    good.release()


# ---- Protocol 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [4, 6], ids=["n16", "n64"])
def test_protocol_one_proofs_join_the_batch(gp, case):
    from bulletproofs_amd.ec import secp256k1
    from bulletproofs_amd.innerproduct import BatchInnerProductVerifier, NIProver, Verifier1
    from bulletproofs_amd.utils import ModP, inner_product
    c = load_golden("ipa.json")["cases"][case]
    n = c["n"]
    s = [bytes.fromhex(x) for x in c["seeds"]]
    g, h = gp.to_gpu_list(gens(n, s[0])), gp.to_gpu_list(gens(n, s[1]))
    u = gp.to_gpu(R.elliptic_hash(s[2]))
    a, b = [gp.gsc(v) for v in scal(n, s[3])], [gp.gsc(v) for v in scal(n, s[4])]
    ip = inner_product(a, b)
    P1 = gp.to_gpu(GoldenPoint(c["P1"]))
    p1 = NIProver(g, h, u, P1, ip, a, b, secp256k1, s[5]).prove()
    assert p1.transcript.decode() == c["proof1"]["transcript"]                  # the golden proof
    assert Verifier1(g, h, u, P1, ip, p1).verify() is True
    others = prove_statements(gp, g, h, n, 2, None, 7 + n)
    eng = gp.engine()

    def batch(u_, P_, c_, proof1):
        bv = BatchInnerProductVerifier(g, h, engine=eng)
        assert bv.add(others[0].u, others[0].P, others[0].proof) == 0
        assert bv.add_proof1(u_, P_, c_, proof1) == 1
        assert bv.add(others[1].u, others[1].P, others[1].proof) == 2
        verdict, where = bv.verify(), bv.locate()
        bv.release()
        return verdict, where

    assert batch(u, P1, ip, p1) == (True, [])
    assert batch(u, P1, ip + ModP(1, Q), p1) == (False, [1])
    assert batch(u, 2 * P1, ip, p1) == (False, [1])
    swapped = copy.copy(p1)
    swapped.u_new = u
    assert batch(u, P1, ip, swapped) == (False, [1])
    swapped = copy.copy(p1)
    swapped.P_new = P1
    assert batch(u, P1, ip, swapped) == (False, [1])
    corrupted = copy.copy(p1)
    corrupted.transcript = p1.transcript.replace(p1.transcript.split(b"&")[1], b"1234", 1)
    assert batch(u, P1, ip, corrupted) == (False, [1])


# ---- one large shape --------------------------------------------------------------------------------------------------------------
def test_large_batch_on_the_bucket_pipeline(gp):
    """n = 2^16, three proofs: the MSM of 2 n + 3 x 34 pairs runs on the bucket pipeline, and both halves of a proof's table are 256
    records."""
    from bulletproofs_amd.ec import PackedPoints, secp256k1, unpack_points
    from bulletproofs_amd.utils import ModP
    eng = gp.engine()
    n = 1 << 16
    rnd = random.Random(65536)
    ks = b"".join(rnd.randrange(1, Q).to_bytes(32, "little") for _ in range(2 * n))
    raw = eng.ec_mul_batch_bytes(secp256k1.G.to_le64() * (2 * n), ks, 2 * n)
    g, h = PackedPoints(unpack_points(raw[: 64 * n], n), raw[: 64 * n]), PackedPoints(unpack_points(raw[64 * n:], n), raw[64 * n:])
    assert eng.msm_geometry(2 * n + 3 * 34)["kernel"] == "pipeline"
    sts = prove_statements(gp, g, h, n, 3, None, 16)
    bv = make_verifier(gp, g, h, None, sts)
    assert bv.verify() is True
    bv.release()
    bad = Statement(sts[1].u, sts[1].P, copy.copy(sts[1].proof))
    bad.proof.a = sts[1].proof.a + ModP(1, Q)
    bv = make_verifier(gp, g, h, None, [sts[0], bad, sts[2]])
    assert bv.verify() is False and bv.locate() == [1]
    bv.release()


# ---- argument errors --------------------------------------------------------------------------------------------------------------
def test_argument_errors_of_the_batch_entry_points(gp):
    eng = gp.engine()
    lib, ctx = eng.lib, eng.ctx
    n, k = 4, 2
    pts, _ = gp.rand_points(2 * n + 3, 11)
    d_g, d_h = eng.upload(cbind.pack_points(pts[:n])), eng.upload(cbind.pack_points(pts[n: 2 * n]))
    xs = pack([3, 5])
    xi = pack([pow(3, -1, Q), pow(5, -1, Q)])
    one = pack([1])
    ex_pts, ex_sc = cbind.pack_points(pts[2 * n:]), pack([1, 2, 3])

    def call(dg=None, dh=None, n_=n, proofs=1, xs_=xs, xi_=xi, k_=k, a=one, b=one, w=one, ep=ex_pts, es=ex_sc, ne=3, no_out=False):
        out = ctypes.create_string_buffer(64)
        rc = lib.bpmi_ipa_verify_batch_dev(ctx, d_g.ptr if dg is None else dg, d_h.ptr if dh is None else dh, None, n_, proofs, xs_, xi_, k_, a, b, w,
                                           ep, es, ne, None if no_out else out)
        return rc, lib.bpmi_last_error(ctx).decode(), out.raw

    try:
        rc, _, out = call()
        assert rc == 0 and out != bytes(64)                                    # a well-formed call (of an invalid statement)
        for kw, text in [(dict(n_=3), "2^k"), (dict(n_=8), "k of the challenge"), (dict(k_=3), "k of the challenge"), (dict(proofs=0), "2^16 proofs"),
                         (dict(proofs=(1 << 16) + 1), "2^16 proofs"), (dict(n_=1 << 22, k_=22, proofs=1025), "2^32"),
                         (dict(n_=1 << 23, k_=23), "k <= 22"), (dict(ne=(1 << 22) + 1), "2^22 extra"),
                         (dict(dg=0), "null"), (dict(dh=0), "null"), (dict(a=None), "null"), (dict(b=None), "null"), (dict(w=None), "null"),
                         (dict(xs_=None), "null"), (dict(xi_=None), "null"), (dict(ep=None), "null"), (dict(es=None), "null"), (dict(no_out=True), "null")]:
            rc, msg, out = call(**kw)
            assert rc == -3 and text in msg, (kw, msg)
            assert out == bytes(64)                                            # refused before anything is done: `out` is not written
        # an extra point off the curve: BPMI_E_ARG naming its index, and `out` is not the identity
        bad = bytearray(ex_pts)
        bad[64 + 32] ^= 1
        rc, msg, out = call(ep=bytes(bad))
        assert rc == -3 and "extra_pts[1]" in msg and "bpmi_ipa_verify_batch_dev" in msg and out != bytes(64)
        # 65 extra points, the smallest count the kernel checks instead of the host: the same refusal.  From level 2 the generators are
        # checked too, and of several bad arrays the first in the order d_g, d_h, extra_pts is named
        text, refused = "bpmi_ipa_verify_batch_dev: %s is not a point of the curve", b"\xff" * 64

        def flipped(blob, i):
            b = bytearray(blob)
            b[64 * i + 32] ^= 1
            return bytes(b)
        g_bytes, h_bytes = cbind.pack_points(pts[:n]), cbind.pack_points(pts[n: 2 * n])
        ex65, es65 = cbind.pack_points(gp.rand_points(65, 12)[0]), pack(list(range(1, 66)))
        rc, _, out = call(ep=ex65, es=es65, ne=65)
        assert rc == 0 and out not in (bytes(64), refused)
        assert call(ep=flipped(ex65, 64), es=es65, ne=65) == (-3, text % "extra_pts[64]", refused)
        d_g.upload(flipped(g_bytes, 3))
        assert call()[0] == 0                                                  # level 1: device pointers are the caller's responsibility
        eng.set_option("validate_points", 2)
        assert call(ep=flipped(ex65, 64), es=es65, ne=65) == (-3, text % "d_g[3]", refused)
        d_g.upload(g_bytes)
        d_h.upload(flipped(h_bytes, 2))
        assert call() == (-3, text % "d_h[2]", refused)
        d_h.upload(h_bytes)
        assert call()[0] == 0
        eng.set_option("validate_points", 1)
        sa, sb = ctypes.create_string_buffer(32 * n), ctypes.create_string_buffer(32 * n)
        assert lib.bpmi_sc_svector_sum(ctx, k, 0, xs, xi, one, one, one, None, sa, sb) == -3 and "2^16 proofs" in lib.bpmi_last_error(ctx).decode()
        assert lib.bpmi_sc_svector_sum(ctx, 23, 1, xs, xi, one, one, one, None, sa, sb) == -3 and "k <= 22" in lib.bpmi_last_error(ctx).decode()
        assert lib.bpmi_sc_svector_sum(ctx, k, 1, xs, xi, one, one, None, None, sa, sb) == -3 and "null" in lib.bpmi_last_error(ctx).decode()
        assert lib.bpmi_sc_svector_sum(ctx, k, 1, xs, xi, one, one, one, None, sa, None) == -3
        assert lib.bpmi_sc_svector_sum(None, k, 1, xs, xi, one, one, one, None, sa, sb) == -3
        assert lib.bpmi_sc_svector_sum(ctx, k, 1, xs, xi, one, one, one, None, sa, sb) == 0
    finally:
        eng.set_option("validate_points", 1)
        d_g.free()
        d_h.free()
