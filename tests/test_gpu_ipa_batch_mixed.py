"""GPU tests of the batch verifier of inner-product proofs of DIFFERENT lengths over the prefixes of one generator list: the weighted
s-vector sums (bpmi_sc_svector_sum_mixed) against Python integers and, for one length, against bpmi_sc_svector_sum byte for byte;
MixedBatchInnerProductVerifier end to end against Verifier2 / Verifier1 proof by proof over the prefixes; the random weights; and the
argument errors of the two entry points."""
import copy
import ctypes
import functools
import random

import pytest

from helpers import Q
from ipa_mixed_ref import LENGTH_LISTS, MORE_LISTS, draw_mixed, draw_scale_mixed, n_gens_of, ref_sums_mixed
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


# ---- bpmi_sc_svector_sum_mixed ------------------------------------------------------------------------------------------------------
LISTS = LENGTH_LISTS + MORE_LISTS


def list_id(ks):
    return "%dx%s" % (len(ks), "k%d" % ks[0] if len(set(ks)) == 1 else "mixed%d" % max(ks))


@functools.lru_cache(maxsize=None)
def sum_case(at):
    ks = LISTS[at]
    ps = draw_mixed(ks, 400 + at)
    scale = draw_scale_mixed(ks, n_gens_of(ks), 50 + at)
    return ks, ps, scale, ref_sums_mixed(ks, ps)


def mixed_call(eng, n_gens, ks, ps, scale=None):
    sa, sb = eng.sc_svector_sum_mixed_bytes(n_gens, ks, pack([x for p in ps for x in p[0]]), pack([pow(x, -1, Q) for p in ps for x in p[0]]),
                                            pack([p[1] for p in ps]), pack([p[2] for p in ps]), pack([p[3] for p in ps]),
                                            None if scale is None else pack(scale))
    return sa, sb


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scale"])
@pytest.mark.parametrize("at", range(len(LISTS)), ids=[list_id(ks) for ks in LISTS])
def test_mixed_sums_equal_python_integers(gp, at, scaled):
    ks, ps, scale, (sa, sb) = sum_case(at)
    n_top = 1 << max(ks)
    assert any(p[1] == 0 for p in ps) and (max(ks.count(k) for k in ks) < 2 or any(p[2] == 0 for p in ps))       # a = 0, b = 0 among the proofs
    assert scale[0] == 1 and (n_top == 1 or scale[n_top - 1] == 0) and len(scale) == n_gens_of(ks)
    eng = gp.engine()
    raw_a, raw_b = mixed_call(eng, n_gens_of(ks), ks, ps, scale if scaled else None)
    assert len(raw_a) == len(raw_b) == 32 * n_top
    assert unpack(raw_a) == sa
    assert unpack(raw_b) == ([v * c % Q for v, c in zip(sb, scale)] if scaled else sb)
    if len(set(ks)) == 1:                                    # one length: the bytes of the existing call
        k = ks[0]
        assert (raw_a, raw_b) == eng.sc_svector_sum_bytes(k, len(ps), pack([x for p in ps for x in p[0]]), pack([pow(x, -1, Q) for p in ps for x in p[0]]),
                                                          pack([p[1] for p in ps]), pack([p[2] for p in ps]), pack([p[3] for p in ps]),
                                                          pack(scale[:n_top]) if scaled else None)


def test_the_order_of_the_caller_is_free(gp):
    """The same proofs in another order: the same sums."""
    ks, ps, scale, (sa, sb) = sum_case(1)                    # [3, 0, 1, 3, 2]
    order = [4, 2, 0, 3, 1]
    raw_a, raw_b = mixed_call(gp.engine(), 8, [ks[i] for i in order], [ps[i] for i in order])
    assert (unpack(raw_a), unpack(raw_b)) == (sa, sb)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
CAPACITY = 64
# elements per statement; "1": through Protocol 1 (add_proof1).  The longest are 2 (Protocol 2) and 5 (Protocol 1)
SHAPES = [(8, 2), (1, 2), (64, 2), (2, 1), (8, 2), (64, 1), (2, 2), (1, 2)]


class Statement:
    def __init__(self, n, u, P, proof, c=None):
        self.n, self.u, self.P, self.proof, self.c = n, u, P, proof, c


def single_verdict(g, h, scale, st):
    from bulletproofs_amd.innerproduct import Verifier1, Verifier2
    gs, hs, cs = list(g)[: st.n], list(h)[: st.n], None if scale is None else scale[: st.n]
    try:
        if st.c is None:
            return Verifier2(gs, hs, st.u, st.P, st.proof, cs).verify() is True
        return Verifier1(gs, hs, st.u, st.P, st.c, st.proof, cs).verify() is True
    except Exception as e:
        assert "Proof invalid" in str(e)
        return False


def prove(gp, g, h, scale, n, protocol, u, rnd):
    from bulletproofs_amd.ec import secp256k1
    from bulletproofs_amd.innerproduct import FastNIProver2, NIProver
    from bulletproofs_amd.utils import ModP, inner_product, vector_commitment
    gs, hs, cs = list(g)[:n], list(h)[:n], None if scale is None else scale[:n]
    a = [ModP(rnd.randrange(Q), Q) for _ in range(n)]
    b = [ModP(rnd.randrange(Q), Q) for _ in range(n)]
    bs = b if cs is None else [v * c for v, c in zip(b, cs)]
    ip = inner_product(a, b)
    if protocol == 2:
        Pt = vector_commitment(gs, hs, a, bs) + ip * u
        return Statement(n, u, Pt, FastNIProver2(gs, hs, u, Pt, a, b, secp256k1, h_scale=cs).prove())
    Pt = vector_commitment(gs, hs, a, bs)
    return Statement(n, u, Pt, NIProver(gs, hs, u, Pt, ip, a, b, secp256k1, b"seed-%d" % n, h_scale=cs).prove(), ip)


@pytest.fixture(scope="module")
def world(gp):
    """scaled -> (g, h, scale, the eight valid statements), proved once over prefixes of ONE list of 64 generators."""
    pts = gp.to_gpu_list(gp.rand_points(2 * CAPACITY + len(SHAPES), 6464)[0])
    g, h, us = pts[:CAPACITY], pts[CAPACITY: 2 * CAPACITY], pts[2 * CAPACITY:]
    made = {}

    def get(scaled):
        if scaled not in made:
            rnd = random.Random(64 + scaled)
            scale = [rnd.randrange(1, Q) for _ in range(CAPACITY)] if scaled else None
            made[scaled] = (g, h, scale, [prove(gp, g, h, scale, n, protocol, us[i], rnd) for i, (n, protocol) in enumerate(SHAPES)])
        return made[scaled]
    return get


def make_verifier(gp, g, h, scale, sts, calls=None):
    from bulletproofs_amd.innerproduct import MixedBatchInnerProductVerifier
    eng = gp.engine()
    bv = MixedBatchInnerProductVerifier(g, h, scale, engine=eng)
    if calls is not None:
        inner = eng.ipa_verify_batch_mixed_dev

        class Counting:
            def __getattr__(self, name):
                return getattr(eng, name)

            def ipa_verify_batch_mixed_dev(self, *a, **kw):
                calls.append(list(a[3]))                     # the round counts of the call
                return inner(*a, **kw)
        bv.engine = Counting()
    for i, s in enumerate(sts):
        assert (bv.add(s.u, s.P, s.proof) if s.c is None else bv.add_proof1(s.u, s.P, s.c, s.proof)) == i
    return bv


def tampered(kind, s):
    from bulletproofs_amd.utils import ModP
    m = Statement(s.n, s.u, s.P, copy.copy(s.proof), s.c)
    if kind == "a":
        m.proof.a = s.proof.a + ModP(1, Q)
    elif kind == "L":
        m.proof.Ls = [s.proof.Rs[0]] + list(s.proof.Ls[1:])
    elif kind == "P":
        m.P = s.P + s.u
    elif kind == "u_new":
        m.proof.u_new = s.u
    return m


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scale"])
def test_mixed_batch_accepts_valid_proofs_and_names_a_tampered_one(gp, world, scaled):
    from bulletproofs_amd.innerproduct import batch_verify_inner_products_mixed
    g, h, scale, sts = world(scaled)
    assert all(single_verdict(g, h, scale, s) for s in sts)
    calls = []
    bv = make_verifier(gp, g, h, scale, sts, calls)
    assert len(bv) == 8 and bv.verify() is True
    assert calls == [[3, 0, 6, 1, 3, 6, 1, 0]]               # ONE native call over all the lengths, the caller's order
    assert bv.locate() == []
    bv.release()
    assert batch_verify_inner_products_mixed(g, h, [(s.u, s.P, s.proof) for s in sts if s.c is None], h_scale=scale, engine=gp.engine()) is True
    # each of a, an L, P and a Protocol-1 u_new in turn, on a short proof and on the longest
    for kind, at in [("a", 1), ("a", 2), ("L", 6), ("L", 2), ("P", 7), ("P", 2), ("u_new", 3), ("u_new", 5)]:
        mixed = list(sts)
        mixed[at] = tampered(kind, sts[at])
        assert single_verdict(g, h, scale, mixed[at]) is False, (kind, at)
        bv = make_verifier(gp, g, h, scale, mixed)
        assert bv.verify() is False, (kind, at)
        assert bv.locate() == [at], (kind, at)
        bv.release()


def test_errors_of_different_lengths_cancel_only_under_known_weights(gp, world):
    """P_1 + u on a proof of 2 elements, P_2 - u on one of 64: they cancel under the weights (1, 1) -- the reason the weights must be
    random -- and under no others."""
    g, h, _, _ = world(False)
    rnd = random.Random(5)
    u = gp.to_gpu(gp.rand_points(1, 77)[0][0])
    s1, s2 = prove(gp, g, h, None, 2, 2, u, rnd), prove(gp, g, h, None, 64, 2, u, rnd)
    bad = [Statement(2, u, s1.P + u, s1.proof), Statement(64, u, s2.P - u, s2.proof)]
    assert not single_verdict(g, h, None, bad[0]) and not single_verdict(g, h, None, bad[1])
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


def test_a_proof_longer_than_the_capacity_is_invalid_on_the_host(gp, world):
    g, h, _, sts = world(False)
    calls = []
    bv = make_verifier(gp, g[:8], h[:8], None, [sts[0], sts[2], sts[1]], calls)          # 8, 64 and 1 elements over a capacity of 8
    assert bv.verify() is False and calls == []              # refused before anything reaches the device
    assert bv.locate() == [1] and calls and all(max(c) <= 3 for c in calls)        # the probes run over the proofs that passed the host checks
    bv.reset()
    assert len(bv) == 0 and bv.verify() is True and bv.locate() == []                    # an empty batch
    assert bv.add(sts[0].u, sts[0].P, sts[0].proof) == 0 and bv.verify() is True
    bv.release()


# ---- argument errors --------------------------------------------------------------------------------------------------------------
def test_argument_errors_of_the_mixed_entry_points(gp):
    eng = gp.engine()
    lib, ctx = eng.lib, eng.ctx
    n = 4
    pts, _ = gp.rand_points(2 * n + 3, 11)
    d_g, d_h = eng.upload(cbind.pack_points(pts[:n])), eng.upload(cbind.pack_points(pts[n: 2 * n]))
    xs = pack([3, 5, 7])
    xi = pack([pow(3, -1, Q), pow(5, -1, Q), pow(7, -1, Q)])
    two = pack([1, 1])
    ex_pts, ex_sc = cbind.pack_points(pts[2 * n:]), pack([1, 2, 3])
    refused = b"\xff" * 64

    def u32s(ks):
        return (ctypes.c_uint32 * max(len(ks), 1))(*ks)

    def call(dg=None, dh=None, n_=n, ks=(2, 1), no_ks=False, xs_=xs, xi_=xi, a=two, b=two, w=two, ep=ex_pts, es=ex_sc, ne=3, no_out=False):
        out = ctypes.create_string_buffer(64)
        rc = lib.bpmi_ipa_verify_batch_mixed_dev(ctx, d_g.ptr if dg is None else dg, d_h.ptr if dh is None else dh, None, n_, len(ks), None if no_ks else u32s(ks),
                                                 xs_, xi_, a, b, w, ep, es, ne, None if no_out else out)
        return rc, lib.bpmi_last_error(ctx).decode(), out.raw

    try:
        rc, _, out = call()
        assert rc == 0 and out not in (bytes(64), refused)                     # a well-formed call (of an invalid statement)
        for kw, text in [(dict(n_=3), "2^K"), (dict(n_=0), "2^K"), (dict(n_=1 << 23), "K <= 22"), (dict(ks=(2, 3)), "at most K"), (dict(ks=()), "2^16 proofs"),
                         (dict(ks=(0,) * ((1 << 16) + 1)), "2^16 proofs"), (dict(n_=1 << 22, ks=(22,) * 1025), "2^32"),
                         (dict(n_=1 << 15, ks=(15,) * 43691), "1 GiB"), (dict(ne=(1 << 22) + 1), "2^22 extra"),
                         (dict(dg=0), "null"), (dict(dh=0), "null"), (dict(no_ks=True), "null"), (dict(a=None), "null"), (dict(b=None), "null"), (dict(w=None), "null"),
                         (dict(xs_=None), "null"), (dict(xi_=None), "null"), (dict(ep=None), "null"), (dict(es=None), "null"), (dict(no_out=True), "null")]:
            rc, msg, out = call(**kw)
            assert rc == -3 and text in msg, (kw if len(str(kw)) < 80 else text, msg)
            assert out == bytes(64)                                            # refused before anything is done: `out` is not written
        assert "bpmi_ipa_verify_batch_mixed_dev" in call(n_=3)[1]
        assert call(ks=(0, 0), xs_=None, xi_=None)[0] == 0                     # no challenges at all: the arrays may be missing
        # an extra point off the curve: BPMI_E_ARG naming its index, and 0xFF.. in `out`
        bad = bytearray(ex_pts)
        bad[64 + 32] ^= 1
        rc, msg, out = call(ep=bytes(bad))
        assert rc == -3 and "extra_pts[1]" in msg and "bpmi_ipa_verify_batch_mixed_dev" in msg and out == refused
        # 65 extra points: checked by the kernel, the same refusal.  From level 2 the generators the MSM reads are checked too
        text = "bpmi_ipa_verify_batch_mixed_dev: %s is not a point of the curve"

        def flipped(blob, i):
            b = bytearray(blob)
            b[64 * i + 32] ^= 1
            return bytes(b)
        g_bytes = cbind.pack_points(pts[:n])
        ex65, es65 = cbind.pack_points(gp.rand_points(65, 12)[0]), pack(list(range(1, 66)))
        rc, _, out = call(ep=ex65, es=es65, ne=65)
        assert rc == 0 and out not in (bytes(64), refused)
        assert call(ep=flipped(ex65, 64), es=es65, ne=65) == (-3, text % "extra_pts[64]", refused)
        d_g.upload(flipped(g_bytes, 3))
        assert call()[0] == 0                                                  # level 1: device pointers are the caller's responsibility
        eng.set_option("validate_points", 2)
        assert call() == (-3, text % "d_g[3]", refused)
        assert call(ks=(1, 1), xs_=xs[:64], xi_=xi[:64])[0] == 0               # n_top = 2: generator 3 is not read, and not checked
        d_g.upload(g_bytes)
        assert call()[0] == 0
        eng.set_option("validate_points", 1)
        sa, sb, n_top = ctypes.create_string_buffer(32 * n), ctypes.create_string_buffer(32 * n), ctypes.c_uint64(99)

        def sums(ctx_=ctx, n_=n, ks=(2, 1), w=two, sb_=sb, nt=ctypes.byref(n_top)):
            rc = lib.bpmi_sc_svector_sum_mixed(ctx_, n_, len(ks), u32s(ks), xs, xi, two, two, w, None, sa, sb_, nt)
            return rc, lib.bpmi_last_error(ctx).decode()
        for kw, text in [(dict(ks=()), "2^16 proofs"), (dict(n_=1 << 23), "K <= 22"), (dict(ks=(3, 1)), "at most K"), (dict(n_=1 << 22, ks=(22,) * 1025), "2^32"),
                         (dict(n_=1 << 15, ks=(15,) * 43691), "1 GiB"), (dict(w=None), "null"), (dict(sb_=None), "null"), (dict(nt=None), "null")]:
            rc, msg = sums(**kw)
            assert rc == -3 and text in msg and n_top.value == 99, (text, msg)
        assert sums(ctx_=None)[0] == -3
        assert sums()[0] == 0 and n_top.value == 4
        assert sums(ks=(1, 0))[0] == 0 and n_top.value == 2
    finally:
        eng.set_option("validate_points", 1)
        d_g.free()
        d_h.free()
