"""GPU parity of the batched inner-product prover's MIXED calls (bpmi_ipa_prove_batch_mixed, bpmi_ipa_batch_prover_commit_batch_mixed,
innerproduct/batch_prover_mixed.py): one prover over N generators proves classes of different lengths n_c <= N in one call, and every
class is byte for byte what a BatchInnerProductProver created over g[:n_c], h[:n_c], u, h_scale[:n_c] writes -- which
tests/test_gpu_ipa_prove_batch.py pins to NIProver / FastNIProver2 and to the reference's goldens -- and the goldens directly
(tests/golden/ipa.json, all nine lengths from ONE prover in ONE call); the statements of the classes equal commit_packed of the prefix
prover, the classes pass MixedBatchInnerProductVerifier, and the C ABI refuses what include/bpmi.h says it refuses.

The tables are built with 6-bit windows (180 MB at N = 1 024); every prover is closed in `finally`.  The prefix provers' outputs of the
shapes of section 2 are computed once per module and shared."""
import ctypes
import os
import random
import subprocess
from base64 import b64encode

import pytest

from conftest import load_golden
from helpers import P as OP, Q, gens, hx, scal
from oracle import bp_ref as R

pytestmark = pytest.mark.gpu

E_ARG = -3
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gp():
    import gpu_common
    return gpu_common


def _points(gp, count, seed):
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


def _inner(a, b):
    from bulletproofs_amd.utils import ModP
    return ModP(sum(x.x * y.x for x, y in zip(a, b)) % Q, Q)


def f2(p):
    return (p.a.x, p.b.x, [x.x for x in p.xs], [pt.to_le64() for pt in p.Ls], [pt.to_le64() for pt in p.Rs], p.transcript, p.start_transcript)


def f1(p):
    return (p.u_new.to_le64(), p.P_new.to_le64(), p.transcript) + f2(p.proof2)


class _Options:
    """engine options for the length of a block, restored afterwards"""

    def __init__(self, eng, **opts):
        self.eng, self.opts = eng, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.eng.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.eng.set_option(k, 0)


def _mixed(gp, g, h, u, h_scale=None):
    from bulletproofs_amd.innerproduct import MixedBatchInnerProductProver
    with _Options(gp.engine(), prover_table_bits=6):
        return MixedBatchInnerProductProver(g, h, u, h_scale=h_scale)


def _prefix(gp, g, h, u, n, h_scale=None):
    from bulletproofs_amd.innerproduct import BatchInnerProductProver
    with _Options(gp.engine(), prover_table_bits=6):
        return BatchInnerProductProver(g[:n], h[:n], u, h_scale=None if h_scale is None else h_scale[:n])


class _Class:
    """one class of a test: its inputs, and what the prefix prover writes for them"""

    def __init__(self, n, count, seed, Ps):
        self.n, self.count, self.Ps = n, count, Ps
        self.As, self.Bs = _vectors(n, count, 7 * seed + n), _vectors(n, count, 11 * seed + n)
        self.cs = [_inner(a, b) for a, b in zip(self.As, self.Bs)]
        self.seeds, self.prefixes = _seeds(count, random.Random(seed)), _prefixes(count)
        self.ts = _vectors(1, count, 13 * seed)
        self.ts = [t[0] for t in self.ts]

    def reference(self, bp, c_given=True, drop=None):
        """drop: "a" / "b" -- the half the statements without a u term and with given ts leave out"""
        self.c_given, self.drop = c_given, drop
        self.want1 = bp.prove1_packed(self.Ps, self.cs if c_given else None, self.As, self.Bs, self.seeds)
        self.want2 = bp.prove2_packed(self.As, self.Bs, self.prefixes)
        as_, bs = (None if drop == "a" else self.As), (None if drop == "b" else self.Bs)
        self.want_commit = {None: bp.commit_packed(as_, bs), "inner": bp.commit_packed(self.As, self.Bs, "inner"), "given": bp.commit_packed(as_, bs, self.ts)}

    def args1(self):
        return (self.n, self.Ps, self.cs if self.c_given else None, self.As, self.Bs, self.seeds)

    def args2(self):
        return (self.n, self.As, self.Bs, self.prefixes)

    def commit_args(self, mode):
        if mode == "inner":
            return (self.n, self.As, self.Bs)
        as_, bs = (None if self.drop == "a" else self.As), (None if self.drop == "b" else self.Bs)
        return (self.n, as_, bs) + ((self.ts,) if mode == "given" else ())


def _build(gp, N, shapes, seed, h_scale=None, edit=None):
    """(mixed prover, classes with their references) over a capacity of N; the prefix provers are closed here.  c is given in the even
    classes and NULL in the odd ones; class 2 leaves as_ out of its statements, class 3 bs."""
    pts = _points(gp, 2 * N + 1 + sum(c for _, c in shapes), seed)
    g, h, u, extra = pts[:N], pts[N: 2 * N], pts[2 * N], pts[2 * N + 1:]
    if edit:
        edit(g, h)
    classes, at = [], 0
    for i, (n, count) in enumerate(shapes):
        classes.append(_Class(n, count, seed + i, extra[at: at + count]))
        at += count
    provers = {}
    try:
        for i, cl in enumerate(classes):
            if cl.n not in provers:
                provers[cl.n] = _prefix(gp, g, h, u, cl.n, h_scale)
            cl.reference(provers[cl.n], c_given=i % 2 == 0, drop={2: "a", 3: "b"}.get(i))
    finally:
        for bp in provers.values():
            bp.close()
    return _mixed(gp, g, h, u, h_scale), classes, (g, h, u)


def _assert_classes(mp, classes):
    got1 = mp.prove1_classes_packed([cl.args1() for cl in classes])
    got2 = mp.prove2_classes_packed([cl.args2() for cl in classes])
    assert len(got1) == len(got2) == len(classes)
    for i, cl in enumerate(classes):
        for name, got, want in zip(("ab", "xs", "lr", "head", "transcripts"), got1[i], cl.want1):
            assert got == want, ("protocol 1", i, cl.n, name)
        for name, got, want in zip(("ab", "xs", "lr", "transcripts"), got2[i], cl.want2):
            assert got == want, ("protocol 2", i, cl.n, name)
    return got1, got2


# ---- 1. the reference's goldens from one prover in one call ------------------------------------------------------------------
def _check_golden2(gp, p2, want):
    assert hx(p2.a.x) == want["a"] and hx(p2.b.x) == want["b"]
    assert [hx(x.x) for x in p2.xs] == want["xs"]
    assert len(p2.Ls) == len(want["Ls"]) and all(gp.same_point(a, OP(b)) for a, b in zip(p2.Ls, want["Ls"]))
    assert len(p2.Rs) == len(want["Rs"]) and all(gp.same_point(a, OP(b)) for a, b in zip(p2.Rs, want["Rs"]))
    assert p2.transcript.decode() == want["transcript"]
    assert p2.start_transcript == want["start_transcript"]


def test_reference_goldens_from_one_prover_in_one_call(gp):
    """The nine cases n = 1 .. 256 of tests/golden/ipa.json share their seeds and the generators are prefix-stable: nine classes over the
    prefixes of ONE list of 256 generators, two copies each, one Protocol-2 call and one Protocol-1 call."""
    cases = load_golden("ipa.json")["cases"][:9]
    assert [c["n"] for c in cases] == [1 << k for k in range(9)] and all(c["seeds"] == cases[0]["seeds"] for c in cases)
    s = [bytes.fromhex(x) for x in cases[0]["seeds"]]
    N = 256
    g, h, u = gp.to_gpu_list(gens(N, s[0])), gp.to_gpu_list(gens(N, s[1])), gp.to_gpu(R.elliptic_hash(s[2]))
    a, b = [gp.gsc(v) for v in scal(N, s[3])], [gp.gsc(v) for v in scal(N, s[4])]
    items2, items1 = [], []
    for c in cases:
        n = c["n"]
        ip = _inner(a[:n], b[:n])
        assert hx(ip.x) == c["c"]
        items2 += [(a[:n], b[:n], None)] * 2
        items1 += [(gp.to_gpu(OP(c["P1"])), ip, a[:n], b[:n], s[5])] * 2
    mp = _mixed(gp, g, h, u)
    try:
        got2, got1 = mp.prove2(items2), mp.prove1(items1)
    finally:
        mp.close()
    for i, c in enumerate(cases):
        for p2 in got2[2 * i: 2 * i + 2]:
            _check_golden2(gp, p2, c["proof2"])
        for p1 in got1[2 * i: 2 * i + 2]:
            assert gp.same_point(p1.u_new, OP(c["proof1"]["u_new"])) and gp.same_point(p1.P_new, OP(c["proof1"]["P_new"]))
            assert p1.transcript.decode() == c["proof1"]["transcript"]
            _check_golden2(gp, p1.proof2, c["proof1"]["proof2"])


# ---- 2. every block shape against the prefix prover --------------------------------------------------------------------------
SHAPES = [(1, 5), (2, 65), (4, 3), (64, 2), (256, 2), (512, 1), (1024, 2), (4, 2)]


@pytest.fixture(scope="module")
def wide(gp):
    """capacity 1 024 with an h_scale whose first entries are 0, 1 and q - 1: zero rounds, a 64-lane chain unit and a job block that
    straddle (2 x 65), per_block 256 .. 1, all three NT instantiations, and a second class of one n"""
    rnd = random.Random(21)
    scale = [0, 1, Q - 1] + [rnd.randrange(1, Q) for _ in range(1021)]
    mp, classes, gens_ = _build(gp, 1024, SHAPES, 2100, h_scale=scale)
    try:
        yield mp, classes, gens_, scale
    finally:
        mp.close()


@pytest.mark.parametrize("job_lanes", [0, 16, 64])
def test_every_block_shape_equals_the_prefix_prover(gp, wide, job_lanes):
    mp, classes, _, _ = wide
    with _Options(gp.engine(), prover_job_lanes=job_lanes):
        _assert_classes(mp, classes)
    ms = mp.last_ms()
    assert ms["total"] > 0 and abs(ms["begin_head"] + ms["rounds"] + ms["copy_out"] - ms["total"]) < 0.05 * ms["total"] + 0.01


# ---- 5. statements -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [None, "inner", "given"])
def test_statements_equal_the_prefix_provers(gp, wide, mode):
    mp, classes, _, _ = wide
    got = mp.commit_classes_packed([cl.commit_args(mode) for cl in classes], mode)
    for i, cl in enumerate(classes):
        assert got[i] == cl.want_commit[mode], (i, cl.n)
    ms = mp.commit_last_ms()
    assert ms["device"] > 0 and ms["call"] >= ms["device"]


def test_the_element_cap_on_the_wide_capacity(gp, wide):
    """2^27 elements: 2^17 proofs of 1 024 elements fill the cap, one more element of another class passes it -- refused from the counts
    alone, before an array is looked at (the pointers here are NULL)."""
    from bulletproofs_amd import _native
    mp = wide[0]
    eng, pv = gp.engine(), mp._bp._handle
    for struct, field, call, arg in ((_native.IpaProveClass, "n_proofs", eng.lib.bpmi_ipa_prove_batch_mixed, 2), (_native.IpaCommitClass, "count", eng.lib.bpmi_ipa_batch_prover_commit_batch_mixed, 0)):
        arr = (struct * 2)()
        arr[0].n, arr[1].n = 1024, 1
        setattr(arr[0], field, 1 << 17)
        setattr(arr[1], field, 1)
        assert call(pv, arg, 2, ctypes.cast(arr, ctypes.c_void_p)) == E_ARG
        assert "at most 2^27 elements (proofs x n) per call" in eng.lib.bpmi_last_error(eng.ctx).decode()
        assert call(pv, arg, 1, ctypes.cast(arr, ctypes.c_void_p)) == E_ARG                     # exactly 2^27 elements pass the cap: the NULL arrays are next
        assert "null argument" in eng.lib.bpmi_last_error(eng.ctx).decode()


# ---- 6. round trip -----------------------------------------------------------------------------------------------------------
def test_round_trip_through_the_mixed_batch_verifier(gp, wide):
    from bulletproofs_amd.innerproduct import MixedBatchInnerProductVerifier
    mp, classes, (g, h, u), scale = wide
    P2 = mp.commit_classes_packed([cl.commit_args("inner") for cl in classes], "inner")
    # (a prefix that does not end in "&", _prefixes' b"raw", runs into the first L of the text: no verifier can split it off again --
    # the reference's included; the round trip takes the kinds that can be verified)
    kinds = (b"", b"one&", b"1&22&333&", None)
    prefixes = [[kinds[i % 4] for i in range(cl.count)] for cl in classes]
    got2 = mp.prove2_classes_packed([(cl.n, cl.As, cl.Bs, prefixes[i]) for i, cl in enumerate(classes)])
    starts = [[len(t.split(b"&")) if t else 1 for t in pre] for pre in prefixes]
    cls2 = [([u] * cl.count, P2[i]) + got2[i] + (starts[i],) for i, cl in enumerate(classes)]
    P1 = mp.commit_classes_packed([(cl.n, cl.As, cl.Bs) for cl in classes])
    got1 = mp.prove1_classes_packed([(cl.n, P1[i], None, cl.As, cl.Bs, cl.seeds) for i, cl in enumerate(classes)])
    cls1 = [(u, P1[i], cl.cs) + got1[i] for i, cl in enumerate(classes)]
    firsts = [sum(c.count for c in classes[:i]) for i in range(len(classes))]
    bv = MixedBatchInnerProductVerifier(g, h, h_scale=scale)
    try:
        assert bv.locate_packed2(cls2, group=None) == [] and bv.verify_packed2(cls2) is True
        assert bv.locate_packed1(cls1, group=None) == [] and bv.verify_packed1(cls1) is True
        # one statement replaced (class 1, proof 40) and one ab byte flipped (class 6, proof 1)
        bad = list(cls2)
        c1 = list(bad[1])
        c1[1] = c1[1][: 64 * 40] + c1[1][64 * 41: 64 * 42] + c1[1][64 * 41:]
        bad[1] = tuple(c1)
        c6 = list(bad[6])
        c6[2] = c6[2][:64] + bytes([c6[2][64] ^ 1]) + c6[2][65:]
        bad[6] = tuple(c6)
        assert bv.verify_packed2(bad) is False
        assert bv.locate_packed2(bad, group=None) == [firsts[1] + 40, firsts[6] + 1]
        b1 = list(cls1)
        c3 = list(b1[3])
        c3[3] = bytes([c3[3][0] ^ 1]) + c3[3][1:]
        b1[3] = tuple(c3)
        assert bv.verify_packed1(b1) is False
    finally:
        bv.release()


def test_prove2_over_shuffled_items_equals_the_single_proof_prover(gp, wide):
    from bulletproofs_amd.ec import secp256k1
    from bulletproofs_amd.innerproduct import FastNIProver2, NIProver
    mp, classes, (g, h, u), scale = wide
    items = []
    for cl in (classes[0], classes[2], classes[3], classes[7]):
        items += [(n_, a, b, t, P, c, sd) for n_, a, b, t, P, c, sd in zip([cl.n] * cl.count, cl.As, cl.Bs, cl.prefixes, cl.Ps, cl.cs, cl.seeds)][:3]
    random.Random(5).shuffle(items)
    assert [it[0] for it in items] != sorted(it[0] for it in items)
    got2 = mp.prove2([(a, b, t) for _, a, b, t, _, _, _ in items])
    got1 = mp.prove1([(P, c, a, b, sd) for _, a, b, _, P, c, sd in items])
    for i, (n, a, b, t, P, c, sd) in enumerate(items):
        want2 = FastNIProver2(g[:n], h[:n], u, P, a, b, secp256k1, t, h_scale=scale[:n]).prove()
        assert f2(got2[i]) == f2(want2), i
        want1 = NIProver(g[:n], h[:n], u, P, c, a, b, secp256k1, sd, h_scale=scale[:n]).prove()
        assert f1(got1[i]) == f1(want1), i


# ---- 3. short capacities -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 8])
def test_short_capacities_with_every_length(gp, N):
    """N = 1: one class, no rounds.  A later call with other classes on the same prover; one class of n = N against
    bpmi_ipa_prove_batch on the SAME prover; single-class, mixed and both statement calls interleaved, each equal to a fresh prover's."""
    lengths = [1 << e for e in range(N.bit_length())]
    shapes = [(n, 3 + i) for i, n in enumerate(lengths)] + [(lengths[0], 2)]
    mp, classes, _ = _build(gp, N, shapes, 3100 + N)
    try:
        _assert_classes(mp, classes)
        later = list(reversed(classes))[:2]
        _assert_classes(mp, later)                                                  # other classes, another order
        top = [cl for cl in classes if cl.n == N][0]
        bp = mp._bp                                                                 # the capacity's own single-class calls
        assert bp.prove2_packed(top.As, top.Bs, top.prefixes) == top.want2
        assert mp.commit_classes_packed([cl.commit_args("inner") for cl in classes], "inner") == [cl.want_commit["inner"] for cl in classes]
        assert bp.prove1_packed(top.Ps, top.cs if top.c_given else None, top.As, top.Bs, top.seeds) == top.want1
        assert mp.prove2_classes_packed([top.args2()]) == [top.want2]
        assert bp.commit_packed(top.As, top.Bs, "inner") == top.want_commit["inner"]
        _assert_classes(mp, classes)
    finally:
        mp.close()


# ---- 4. edges inside the shortest prefixes -----------------------------------------------------------------------------------
def test_degenerate_generators_and_zero_vectors(gp):
    """g_0 the identity, g_1 = h_0, g_2 = -g_3 on a capacity of 8 with classes 2, 4, 8; a = b = 0: every L and R is 64 zero bytes and
    "AA==" in the transcript."""
    from bulletproofs_amd.ec import Point
    from bulletproofs_amd.utils import ModP

    def edit(g, h):
        g[0] = Point.IDENTITY_ELEMENT
        g[1] = h[0]
        g[2] = -g[3]
    mp, classes, _ = _build(gp, 8, [(2, 3), (4, 3), (8, 3)], 4100, edit=edit)
    try:
        _assert_classes(mp, classes)
        zero = lambda n: [[ModP(0, Q)] * n]
        got = mp.prove2_classes_packed([(n, zero(n), zero(n), None) for n in (2, 4, 8)])
        for n, (ab, xs, lr, trs) in zip((2, 4, 8), got):
            k = n.bit_length() - 1
            assert ab == bytes(64) and lr == bytes(128 * k) and trs[0].count(b"AA==&") == 2 * k
    finally:
        mp.close()


def test_the_head_at_the_identity_and_the_doubling_in_a_class(gp):
    """Protocol 1 with P_p the identity, the opposite of (x c) u and equal to it, in the second class of a mixed call."""
    from bulletproofs_amd.ec import Point
    from bulletproofs_amd.pippenger import PipSECP256k1
    from bulletproofs_amd.utils.utils import mod_hash
    N = 8
    pts = _points(gp, 2 * N + 1 + 2, 4200)
    g, h, u = pts[:N], pts[N: 2 * N], pts[2 * N]
    first = _Class(8, 2, 4201, pts[2 * N + 1:])
    edge = _Class(4, 3, 4202, None)
    edge.seeds = [b"", b"head", b"double!"]
    xcu = [PipSECP256k1.multiexp([u], [mod_hash(b64encode(sd) + b"&", Q).x * c.x % Q]) for sd, c in zip(edge.seeds, edge.cs)]
    edge.Ps = [Point.IDENTITY_ELEMENT, -xcu[1], xcu[2]]
    for cl in (first, edge):
        bp = _prefix(gp, g, h, u, cl.n)
        try:
            cl.reference(bp)
        finally:
            bp.close()
    mp = _mixed(gp, g, h, u)
    try:
        got1, _ = _assert_classes(mp, [first, edge])
    finally:
        mp.close()
    head = got1[1][3]
    assert head[64:128] == xcu[0].to_le64() and head[128 + 64: 256] == bytes(64)
    assert head[256 + 64: 384] == PipSECP256k1.multiexp([xcu[2]], [2]).to_le64()


# ---- 7. every refusal of the header ------------------------------------------------------------------------------------------
def test_c_abi_refusals(gp):
    """BPMI_E_ARG, the message naming the class where stated, and every output byte of every class untouched."""
    from bulletproofs_amd import _native
    from bulletproofs_amd.ec import secp256k1
    eng = gp.engine()
    lib = eng.lib
    N, shapes = 8, [(2, 3), (8, 2), (1, 2)]
    total = sum(c for _, c in shapes)
    pts = _points(gp, 2 * N + 1 + total, 7100)
    gb, hb, ub = (b"".join(p.to_le64() for p in pts[:N]), b"".join(p.to_le64() for p in pts[N: 2 * N]), pts[2 * N].to_le64())
    rnd = random.Random(71)
    sc = lambda m: b"".join(rnd.randrange(Q).to_bytes(32, "little") for _ in range(m))
    handle = ctypes.c_void_p()
    with _Options(eng, prover_table_bits=6):
        eng._ck(lib.bpmi_ipa_batch_prover_create(eng.ctx, N, gb, hb, ub, None, ctypes.byref(handle)))
    pv = handle.value
    fill = 0xAB

    def err():
        return lib.bpmi_last_error(eng.ctx).decode()

    addr = lambda b: None if b is None else ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p)
    try:
        assert lib.bpmi_ipa_prove_batch_transcript_bytes_class(pv, 8, 1, 3) == 1 + 4 + 1 + 79 + 3 * 169
        assert lib.bpmi_ipa_prove_batch_transcript_bytes_class(pv, 1, 2, 3) == 4 and lib.bpmi_ipa_prove_batch_transcript_bytes_class(pv, 2, 2, 0) == 1 + 169
        for bad_n in (0, 3, 16):
            assert lib.bpmi_ipa_prove_batch_transcript_bytes_class(pv, bad_n, 1, 0) == 0
        assert lib.bpmi_ipa_prove_batch_transcript_bytes_class(pv, 8, 3, 0) == 0 and lib.bpmi_ipa_prove_batch_transcript_bytes_class(None, 8, 1, 0) == 0
        # the inputs and the poisoned outputs of every class
        data, at = [], 0
        for n, count in shapes:
            k = n.bit_length() - 1
            cap = count * lib.bpmi_ipa_prove_batch_transcript_bytes_class(pv, n, 1, 3)
            poisoned = lambda size: ctypes.create_string_buffer(bytes([fill]) * max(size, 1), max(size, 1))
            data.append(dict(n=n, count=count, a=sc(count * n), b=sc(count * n), c=sc(count), P=b"".join(p.to_le64() for p in pts[2 * N + 1 + at: 2 * N + 1 + at + count]),
                             seeds=b"abcdefgh"[: 3 * count - 1], off=(ctypes.c_uint64 * (count + 1))(*([0, 3, 5, 8][: count + 1])), cap=cap,
                             outs=dict(ab=poisoned(64 * count), xs=poisoned(32 * k * count), LR=poisoned(128 * k * count), head=poisoned(128 * count), transcripts=poisoned(cap)),
                             tr_off=(ctypes.c_uint64 * (count + 1))(*([7] * (count + 1))), out=poisoned(64 * count)))
            at += count

        def untouched():
            return all(buf.raw == bytes([fill]) * len(buf.raw) for d in data for buf in list(d["outs"].values()) + [d["out"]]) and \
                all(list(d["tr_off"]) == [7] * (d["count"] + 1) for d in data)

        def prove(protocol=1, n_classes=None, edits=(), repeat=1):
            """edits: (class, field, value) over the full Protocol-1 call; under protocol 2 c, P and head are NULL unless an edit sets them"""
            keep = []
            arr = (_native.IpaProveClass * (len(data) * repeat))()
            for r in range(repeat):
                for i, d in enumerate(data):
                    v = dict(n=d["n"], n_proofs=d["count"], a=d["a"], b=d["b"], c=d["c"] if protocol == 1 else None, P=d["P"] if protocol == 1 else None, seeds=d["seeds"],
                             seed_off=d["off"], cap=d["cap"], tr_off=d["tr_off"], **d["outs"])
                    if protocol != 1:
                        v["head"] = None
                    for ci, field, value in edits:
                        if ci == i:
                            v[field] = value
                    q = arr[r * len(data) + i]
                    for name, value in v.items():
                        if name in ("n", "n_proofs", "cap"):
                            setattr(q, name, value)
                        elif isinstance(value, (bytes, type(None))):
                            keep.append(value)
                            setattr(q, name, addr(value))
                        else:
                            setattr(q, name, ctypes.addressof(value))
            count = len(data) * repeat if n_classes is None else n_classes
            return lib.bpmi_ipa_prove_batch_mixed(pv, protocol, count, ctypes.cast(arr, ctypes.c_void_p))

        d1, d2 = data[1], data[2]
        refusals = [
            (dict(protocol=0), "protocol must be 1 or 2"), (dict(protocol=3), "protocol must be 1 or 2"),
            (dict(repeat=22), "n_classes must be at most 64"),                                            # 66 classes
            (dict(edits=[(1, "n", 16)]), "class 1: the vector length must be a power of two, at most the prover's"),
            (dict(edits=[(2, "n", 3)]), "class 2: the vector length"), (dict(edits=[(0, "n", 0)]), "class 0: the vector length"),
            (dict(edits=[(1, "n_proofs", 0)]), "class 1: n_proofs must be at least 1"),
            (dict(edits=[(2, "n_proofs", 1 << 20)]), "2^20 proofs"),                                      # 2^20 + 5 in all (nothing of the short arrays is read)
            (dict(edits=[(1, "n_proofs", (1 << 24) - 1), (0, "n_proofs", 1), (2, "n_proofs", 1)]), "2^20 proofs"),
            (dict(edits=[(1, "a", None)]), "class 1: null argument"), (dict(edits=[(0, "b", None)]), "class 0: null argument"),
            (dict(edits=[(1, "P", None)]), "class 1: null argument"), (dict(edits=[(1, "head", None)]), "class 1: null argument"),
            (dict(edits=[(1, "seed_off", None)]), "class 1: null argument"), (dict(edits=[(0, "ab", None)]), "class 0: null argument"),
            (dict(edits=[(1, "xs", None)]), "class 1: null argument"), (dict(edits=[(0, "LR", None)]), "class 0: null argument"),
            (dict(edits=[(2, "transcripts", None)]), "class 2: null argument"), (dict(edits=[(2, "tr_off", None)]), "class 2: null argument"),
            (dict(protocol=2, edits=[(1, "c", d1["c"])]), "class 1: c, P and head must be NULL under Protocol 2"),
            (dict(protocol=2, edits=[(2, "head", d2["outs"]["head"])]), "class 2: c, P and head must be NULL under Protocol 2"),
            (dict(edits=[(1, "seed_off", (ctypes.c_uint64 * 3)(0, 65536, 65536)), (1, "seeds", bytes(65536))]), "class 1: a seed is longer than 65535"),
            (dict(edits=[(0, "seed_off", (ctypes.c_uint64 * 4)(0, 5, 3, 8))]), "class 0: seed offsets must not decrease"),
            (dict(edits=[(1, "seeds", None)]), "class 1: null argument (seeds)"),
            (dict(edits=[(1, "cap", d1["cap"] - 1)]), "class 1: the transcript buffer is too small"), (dict(edits=[(2, "cap", 0)]), "class 2: the transcript buffer is too small"),
            (dict(edits=[(0, "a", data[0]["a"][: 32 * 5] + Q.to_bytes(32, "little"))]), "class 0: a[5] is not below the group order"),
            (dict(edits=[(1, "b", d1["b"][: 32 * 11] + b"\xff" * 32 + d1["b"][32 * 12:])]), "class 1: b[11] is not below the group order"),
            (dict(edits=[(2, "c", d2["c"][:32] + Q.to_bytes(32, "little"))]), "class 2: c[1] is not below the group order"),            # a scalar = q in the LAST class
            (dict(edits=[(2, "a", d2["a"][:32] + Q.to_bytes(32, "little"))]), "class 2: a[1] is not below the group order"),
            (dict(edits=[(1, "P", d1["P"][:64] + (1).to_bytes(32, "little") + (1).to_bytes(32, "little"))]), "class 1: P[1] is not a point of the curve"),   # a bad P in the second
            (dict(edits=[(1, "P", secp256k1.p.to_bytes(32, "little") + bytes(32) + d1["P"][64:])]), "class 1: P[0] is not a point of the curve"),
            (dict(edits=[(2, "P", d2["P"][:64] + (2).to_bytes(32, "little") + (1).to_bytes(32, "little"))]), "class 2: P[1] is not a point of the curve"),
        ]
        for kwargs, text in refusals:
            assert prove(**kwargs) == E_ARG, kwargs
            assert text in err(), (kwargs, err())
            assert "bpmi_ipa_prove_batch_mixed" in err()
            assert untouched(), kwargs
        assert prove(n_classes=0) == 0 and prove(protocol=2, n_classes=0) == 0 and untouched()
        assert lib.bpmi_ipa_prove_batch_mixed(pv, 1, 0, None) == 0 and lib.bpmi_ipa_prove_batch_mixed(pv, 0, 0, None) == E_ARG and "protocol must be 1 or 2" in err()
        assert lib.bpmi_ipa_prove_batch_mixed(pv, 1, 1, None) == E_ARG and "null argument" in err()
        assert lib.bpmi_ipa_prove_batch_mixed(None, 1, 0, None) == E_ARG

        # the statements' call
        def commit(u_mode=0, n_classes=None, edits=()):
            keep = []
            arr = (_native.IpaCommitClass * len(data))()
            for i, d in enumerate(data):
                v = dict(n=d["n"], count=d["count"], a=d["a"], b=d["b"], t=d["c"] if u_mode == 2 else None, out=d["out"])
                for ci, field, value in edits:
                    if ci == i:
                        v[field] = value
                q = arr[i]
                for name, value in v.items():
                    if name in ("n", "count"):
                        setattr(q, name, value)
                    elif isinstance(value, (bytes, type(None))):
                        keep.append(value)
                        setattr(q, name, addr(value))
                    else:
                        setattr(q, name, ctypes.addressof(value))
            return lib.bpmi_ipa_batch_prover_commit_batch_mixed(pv, u_mode, len(data) if n_classes is None else n_classes, ctypes.cast(arr, ctypes.c_void_p))

        commit_refusals = [
            (dict(u_mode=3), "u_mode must be 0"), (dict(u_mode=-1), "u_mode must be 0"),
            (dict(edits=[(1, "n", 16)]), "class 1: the vector length"), (dict(edits=[(2, "count", 0)]), "class 2: n_proofs must be at least 1"),
            (dict(edits=[(2, "count", 1 << 20)]), "2^20 proofs"),
            (dict(edits=[(1, "out", None)]), "class 1: null argument (out)"),
            (dict(edits=[(1, "t", d1["c"])]), "class 1: t must be NULL unless u_mode is 2"), (dict(u_mode=2, edits=[(2, "t", None)]), "class 2: null argument (u_mode 2 takes t)"),
            (dict(edits=[(0, "a", None), (0, "b", None)]), "class 0: a and b are both NULL"), (dict(u_mode=1, edits=[(2, "b", None)]), "class 2: u_mode 1 sums <a, b>"),
            (dict(edits=[(2, "b", d2["b"][:32] + Q.to_bytes(32, "little"))]), "class 2: b[1] is not below the group order"),
            (dict(u_mode=2, edits=[(1, "t", b"\xff" * 64)]), "class 1: t[0] is not below the group order"),
        ]
        for kwargs, text in commit_refusals:
            assert commit(**kwargs) == E_ARG, kwargs
            assert text in err() and "bpmi_ipa_batch_prover_commit_batch_mixed" in err(), (kwargs, err())
            assert untouched(), kwargs
        assert commit(n_classes=0) == 0 and commit(u_mode=3, n_classes=0) == E_ARG and untouched()
        # and the same arrays, accepted
        eng._ck(prove(edits=[(1, "c", None)]))
        assert not untouched() and all(d["tr_off"][0] == 0 and d["tr_off"][d["count"]] <= d["cap"] for d in data)
        assert data[0]["outs"]["transcripts"].raw.startswith(b"&" + b64encode(b"abc") + b"&")
        eng._ck(commit(u_mode=1))
        assert all(d["out"].raw != bytes([fill]) * len(d["out"].raw) for d in data)
    finally:
        lib.bpmi_ipa_batch_prover_destroy(pv)


# ---- 8. the C example --------------------------------------------------------------------------------------------------------
def test_c_example(gp, tmp_path):
    """examples/ipa_prove_mixed_c_abi.c: a C99 program over include/bpmi.h and libbpmi.so alone -- one prover over 64 generators proves
    n = 8 and n = 64 in one call, commits their statements in one call and verifies them with bpmi_ipa_verify_batch_packed_mixed_dev."""
    libdir = os.path.join(REPO, "python-bulletproofs_amd")
    exe = str(tmp_path / "ipa_prove_mixed_c_abi")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"),
                           os.path.join(REPO, "examples", "ipa_prove_mixed_c_abi.c"), "-o", exe, os.path.join(libdir, "libbpmi.so"), "-Wl,-rpath," + libdir,
                           "-Wl,--allow-shlib-undefined"])
    r = subprocess.run([exe, "5", "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "(as proved): VALID" in r.stdout and "(one scalar byte changed): INVALID" in r.stdout
    assert "ok: one prover, one proving call, one statements call, one verifying call" in r.stdout
