"""GPU tests of the batch verifier of PACKED inner-product proofs of DIFFERENT lengths (include/bpmi.h, "a list of classes, one MSM";
csrc/ipa_packed_kernels.hpp: k_ipap_roles_mixed, k_ipap_finish_mixed): the preparation kernels against their host twin byte for byte
(bpmi_ipa_batch_prepare_mixed_dev / bpmi_ipa_batch_prepare_mixed), several rounds against one, the whole call
(bpmi_ipa_verify_batch_packed_mixed_dev) against bpmi_ipa_verify_batch_mixed_dev fed with the twin's output and against the single-class
call, the verdicts of MixedBatchInnerProductVerifier.verify_packed* / locate_packed* against Verifier2 / Verifier1 proof by proof over
each proof's prefix, the capacity rule of the point check, the argument errors and the C example.  The batch provers make the proofs
(prover_table_bits = 4: small tables), one per length, over the prefixes of one list of 64 generators."""
import ctypes
import functools
import os
import random
import subprocess

import pytest

import ipa_packed_ref as PR
from helpers import Q

pytestmark = pytest.mark.gpu

E_ARG = -3
SEED = bytes(range(60, 92))
K, N = 6, 64
PREFIXES = (b"", b"one&", b"1&22&333&", None, b"x" * 90 + b"&")


@pytest.fixture(scope="module")
def gp():
    import gpu_common
    return gpu_common


def _points(count, seed):
    import gpu_common as gp
    from bulletproofs_amd.ec import secp256k1, unpack_points
    rnd = random.Random(seed)
    ks = b"".join(rnd.randrange(1, Q).to_bytes(32, "little") for _ in range(count))
    return unpack_points(gp.engine().ec_mul_batch_bytes(secp256k1.G.to_le64() * count, ks, count), count)


def _vectors(n, count, seed):
    from bulletproofs_amd.utils import ModP
    rnd = random.Random(seed)
    return [[ModP(rnd.randrange(Q), Q) for _ in range(n)] for _ in range(count)]


class Capacity:
    """The one generator list: g, h (64 each), u, and the optional scale."""


@functools.lru_cache(maxsize=None)
def capacity(scaled):
    C = Capacity()
    pts = _points(2 * N + 1, 4242 + scaled)
    C.g, C.h, C.u = pts[:N], pts[N: 2 * N], pts[2 * N]
    C.scale = [random.Random(99).randrange(1, Q) for _ in range(N)] if scaled else None
    return C


@functools.lru_cache(maxsize=None)
def make_class(k, count, protocol, scaled, prefixed, valid_statements):
    """`count` packed proofs of n = 2^k elements from a BatchInnerProductProver over g[:n], h[:n] (, scale[:n]) of the capacity.
    valid_statements: P_i is the commitment the proof is about; otherwise an arbitrary point -- the preparation never looks at the
    group equation."""
    import gpu_common as gp
    from bulletproofs_amd.ec import pack_points
    from bulletproofs_amd.innerproduct import BatchInnerProductProver
    from bulletproofs_amd.utils import ModP, inner_product, vector_commitment
    n = 1 << k
    eng = gp.engine()
    C = capacity(scaled)
    g, h, scale = C.g[:n], C.h[:n], None if C.scale is None else C.scale[:n]
    extra = _points(2 * count, 1000 * k + 7 * protocol + scaled + 13 * count)
    As, Bs = _vectors(n, count, 31 * k + count), _vectors(n, count, 37 * k + count)
    cs = [ModP(sum(x.x * y.x for x, y in zip(a, b)) % Q, Q) for a, b in zip(As, Bs)]
    us = [C.u] * count if protocol == 1 or valid_statements else extra[count:]
    if valid_statements:
        Ps = []
        for i in range(count):
            bs = Bs[i] if scale is None else [v * c for v, c in zip(Bs[i], scale)]
            com = vector_commitment(g, h, As[i], bs)
            Ps.append(com if protocol == 1 else com + inner_product(As[i], Bs[i]) * C.u)
    else:
        Ps = extra[:count]
    eng.set_option("prover_table_bits", 4)
    try:
        bp = BatchInnerProductProver(g, h, C.u, h_scale=scale)
        try:
            pk = PR.Packed(k, protocol)
            pk.count = count
            if protocol == 1:
                seeds = [random.Random(i).randbytes((0, 1, 2, 3, 17, 200)[i % 6]) for i in range(count)]
                ab, xs, lr, head, trs = bp.prove1_packed(Ps, cs, As, Bs, seeds)
                pk.head, pk.c, pk.u = bytearray(head), bytearray(b"".join(PR.le32(c.x) for c in cs)), bytearray(C.u.to_le64())
            else:
                prefixes = [PREFIXES[i % len(PREFIXES)] for i in range(count)] if prefixed else None
                ab, xs, lr, trs = bp.prove2_packed(As, Bs, prefixes)
                pk.u = bytearray(pack_points(us))
                pk.starts = [len(t.split(b"&")) if t else 1 for t in prefixes] if prefixed else None
            pk.ab, pk.xs, pk.lr, pk.trs, pk.P = bytearray(ab), bytearray(xs), bytearray(lr), list(trs), bytearray(pack_points(Ps))
        finally:
            bp.close()
    finally:
        eng.set_option("prover_table_bits", 0)
    return pk


LIST_A = [(1, 3), (6, 65), (0, 1), (3, 130), (3, 64)]          # one lane, a wave plus one, a short last wave, a full wave; k out of order, one k twice
LIST_B = [(6, 1)]


def class_list(shape, protocol, scaled, prefixed, valid=False):
    """The Packed classes of a list of (k, count): classes of one k are disjoint slices of one prover call."""
    need = {}
    for k, count in shape:
        need[k] = need.get(k, 0) + count
    biggest = {6: 65, 3: 194}
    taken, out = {}, []
    for k, count in shape:
        base = make_class(k, max(need[k], biggest.get(k, 0)) if not valid else need[k], protocol, scaled, prefixed, valid)
        lo = taken.get(k, 0)
        out.append(base.subset(list(range(lo, lo + count))))
        taken[k] = lo + count
    return out


def eng_classes(pks):
    return [(pk.k,) + pk.args() for pk in pks]


def explicit_weights(protocol, total, seed):
    rnd = random.Random(seed)
    ws = [[rnd.randrange(1, Q) for _ in range(3 if protocol == 1 else 1)] for _ in range(total)]
    ws[0][0] = Q - 1
    return ws


def host_prepare(protocol, pks, weights=None, seed=None):
    from bulletproofs_amd.engine import ipa_batch_prepare_mixed_host
    return ipa_batch_prepare_mixed_host(K, protocol, eng_classes(pks), weights, seed, 3)


def dev_prepare(gp, protocol, pks, weights=None, seed=None):
    return gp.engine().ipa_batch_prepare_mixed_dev(K, protocol, eng_classes(pks), weights, seed)


NAMES = ("records", "rec_byte_off", "extra_pts", "extra_scalars", "status")


def assert_same(want, got, what=""):
    for name, w_, g_ in zip(NAMES, want, got):
        assert g_ == w_, (what, name)


# ---- 1. the kernels against the host twin --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [LIST_A, LIST_B], ids=["five-classes", "one-proof"])
@pytest.mark.parametrize("protocol", [1, 2])
def test_kernels_equal_the_host_twin_byte_for_byte(gp, protocol, shape):
    """Variant A: plain provers, no prefixes / starts, explicit weights; variant B: provers with h_scale, prefixes and starts (Protocol 2),
    seed-derived weights.  Records, rec_byte_off, extra points, extra scalars, status."""
    for scaled, prefixed in ((False, False), (True, True)):
        pks = class_list(shape, protocol, scaled, prefixed)
        total = sum(pk.count for pk in pks)
        weights, seed = (None, SEED) if scaled else (PR.pack_weights(explicit_weights(protocol, total, 5 + total)), None)
        want, got = host_prepare(protocol, pks, weights, seed), dev_prepare(gp, protocol, pks, weights, seed)
        assert_same(want, got, (protocol, scaled))
        assert want[4] == bytes(total)
        if shape is LIST_A:
            rec = lambda k: 64 * k + 96
            assert want[1] == [rec(6) * 65 + rec(3) * 194, 0, rec(6) * 65 + rec(3) * 194 + rec(1) * 3, rec(6) * 65, rec(6) * 65 + rec(3) * 130]


# ---- 2. rounds ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("protocol", [1, 2])
def test_rounds_give_the_bytes_of_one_round(gp, protocol):
    """A budget below every class's 64 rows: rows = 64 everywhere, so the classes of 130, 65 and 64 (and fewer) proofs take 3, 2 and 1
    rounds -- three launches of k_ipap_roles_mixed with 5, 2 and 1 units."""
    pks = class_list(LIST_A, protocol, True, True)
    want = dev_prepare(gp, protocol, pks, None, SEED)
    eng = gp.engine()
    eng.ipap_t_budget(1000)
    try:
        got = dev_prepare(gp, protocol, pks, None, SEED)
    finally:
        eng.ipap_t_budget(0)
    assert_same(want, got)
    assert_same(host_prepare(protocol, pks, None, SEED), got)


# ---- 3. mutations ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("protocol", [1, 2])
def test_a_batch_of_mutated_proofs_gives_the_same_bytes_on_both_sides(gp, protocol):
    """256 proofs over three classes (k = 3, 1, 6), every one with one random mutation of the tamper table (fixed seed): one call each of
    the twin and the kernels; every status is what the table says."""
    base = class_list([(3, 130), (1, 3), (6, 65)], protocol, False, protocol == 2)
    pks = [base[0].subset([i % 130 for i in range(150)]), base[1].subset([i % 3 for i in range(41)]), base[2].subset(list(range(65)))]
    rows = [t for t in PR.TAMPERS if protocol in t[3]]
    rnd = random.Random(78 + protocol)
    want_status = []
    for pk in pks:
        for i in range(pk.count):
            name, mut, want, _ = rows[rnd.randrange(len(rows))]
            mut(pk, i, rnd)
            want_status.append(want or 0)
    assert len(want_status) == 256
    want, got = host_prepare(protocol, pks, None, SEED), dev_prepare(gp, protocol, pks, None, SEED)
    assert list(want[4]) == want_status and set(want_status) == {0, 1, 2}
    assert_same(want, got)


# ---- 4. the whole call ---------------------------------------------------------------------------------------------------------------------
def make_verifier(gp, scaled, n=N):
    from bulletproofs_amd.innerproduct import MixedBatchInnerProductVerifier
    C = capacity(scaled)
    return MixedBatchInnerProductVerifier(C.g[:n], C.h[:n], h_scale=None if C.scale is None else C.scale[:n], engine=gp.engine())


def mixed_out(gp, bv, protocol, pks, weights=None, seed=None):
    return gp.engine().ipa_verify_batch_packed_mixed_dev(bv._d[0], bv._d[1], bv.n, protocol, eng_classes(pks), weights, seed, bv._d_scale)


VALID_SHAPE = [(1, 2), (3, 3), (0, 1), (2, 2)]


def object_path_inputs(pks, rec, offs):
    """ks class-major; xs, xinvs, a, b, w cut from the records through rec_byte_off."""
    ks, xs, xinvs, a, b, w = [], b"", b"", b"", b"", b""
    for pk, o in zip(pks, offs):
        k, rb = pk.k, 64 * pk.k + 96
        for p in range(pk.count):
            r = rec[o + rb * p: o + rb * (p + 1)]
            ks.append(k)
            xs += b"".join(r[64 * j: 64 * j + 32] for j in range(k))
            xinvs += b"".join(r[64 * j + 32: 64 * j + 64] for j in range(k))
            a, b, w = a + r[64 * k: 64 * k + 32], b + r[64 * k + 32: 64 * k + 64], w + r[64 * k + 64: 64 * k + 96]
    return ks, xs, xinvs, a, b, w


@pytest.mark.parametrize("protocol,scaled", [(2, False), (2, True), (1, False), (1, True)])
def test_out_equals_the_object_path_call_fed_with_the_twins_output(gp, protocol, scaled):
    """Explicit weights; both sides are canonical, so equality is exact -- for a valid batch (the identity) and for one with a wrong a."""
    base = class_list(VALID_SHAPE, protocol, scaled, protocol == 2 and not scaled, valid=True)
    bv = make_verifier(gp, scaled)
    try:
        for wrong in (False, True):
            pks = [pk.clone() for pk in base]
            if wrong:
                PR.mut_a_changed(pks[1], 2, None)
            total = sum(pk.count for pk in pks)
            wb = PR.pack_weights(explicit_weights(protocol, total, 9))
            rec, offs, pts, sc, status = host_prepare(protocol, pks, wb)
            assert status == bytes(total)
            out, st = mixed_out(gp, bv, protocol, pks, wb)
            ks, xs, xinvs, a, b, w = object_path_inputs(pks, rec, offs)
            want = gp.engine().ipa_verify_batch_mixed_dev(bv._d[0], bv._d[1], N, ks, xs, xinvs, a, b, w, pts, sc, len(pts) // 64, bv._d_scale)
            assert st == bytes(total) and out == want
            assert (out == bytes(64)) == (not wrong)
    finally:
        bv.release()


@pytest.mark.parametrize("protocol", [1, 2])
def test_one_class_equals_the_single_class_call(gp, protocol):
    """out and status of a list of one class equal bpmi_ipa_verify_batch_packed_dev's under the same explicit weights (n_gens = n)."""
    (pk,) = class_list([(3, 6)], protocol, False, protocol == 2, valid=True)
    bv = make_verifier(gp, False, n=8)
    try:
        for wrong in (False, True):
            mine = pk.clone()
            if wrong:
                PR.mut_a_changed(mine, 4, None)
                PR.mut_xs_changed(mine, 1, random.Random(1))
            wb = PR.pack_weights(explicit_weights(protocol, 6, 3))
            want = gp.engine().ipa_verify_batch_packed_dev(bv._d[0], bv._d[1], 8, protocol, *mine.args(), wb, None, None)
            got = mixed_out(gp, bv, protocol, [mine], wb)
            assert got == want and (got[0] == bytes(64)) == (not wrong) and list(got[1]) == ([0, 1, 0, 0, 0, 0] if wrong else [0] * 6)
    finally:
        bv.release()


def single_verdicts(scaled, pk):
    """Verifier2.verify / Verifier1.verify over the proof's prefix on the objects built from the same bytes."""
    from bulletproofs_amd.ec import Point
    from bulletproofs_amd.innerproduct import Proof1, Verifier1, Verifier2
    from bulletproofs_amd.innerproduct.batch_prover import BatchInnerProductProver
    from bulletproofs_amd.utils import ModP
    C = capacity(scaled)
    n = 1 << pk.k
    g, h, scale = C.g[:n], C.h[:n], None if C.scale is None else C.scale[:n]
    shim = BatchInnerProductProver.__new__(BatchInnerProductProver)
    shim.k, shim._handle = pk.k, None
    out = []
    for i in range(pk.count):
        try:
            P = Point.from_le64(bytes(pk.P[64 * i: 64 * i + 64]))
            if pk.protocol == 2:
                pr = shim._proof2(i, bytes(pk.ab), bytes(pk.xs), bytes(pk.lr), pk.trs[i], 1 if pk.starts is None else pk.starts[i])
                out.append(Verifier2(g, h, Point.from_le64(bytes(pk.u[64 * i: 64 * i + 64])), P, pr, scale).verify() is True)
            else:
                items = pk.trs[i].split(b"&")
                outer = b"&".join(items[1:3]) + b"&"
                p2 = shim._proof2(i, bytes(pk.ab), bytes(pk.xs), bytes(pk.lr), pk.trs[i], 3)
                head = bytes(pk.head[128 * i: 128 * i + 128])
                p1 = Proof1(Point.from_le64(head[:64]), Point.from_le64(head[64:]), p2, outer)
                c = ModP(PR.from_le(pk.c[32 * i: 32 * i + 32]), Q)
                out.append(Verifier1(g, h, C.u, P, c, p1, scale).verify() is True)
        except Exception:
            out.append(False)
    return out


def api_classes(pks):
    if pks[0].protocol == 2:
        return [(bytes(pk.u), bytes(pk.P), pk.ab, pk.xs, pk.lr, pk.trs, pk.starts) for pk in pks]
    return [(bytes(pk.u), bytes(pk.P), bytes(pk.c), pk.ab, pk.xs, pk.lr, pk.head, pk.trs) for pk in pks]


@pytest.mark.parametrize("protocol,scaled", [(2, False), (1, True)])
def test_verdicts_and_located_indices_equal_the_single_proof_verifiers(gp, protocol, scaled):
    base = class_list(VALID_SHAPE, protocol, scaled, False, valid=True)
    bv = make_verifier(gp, scaled)
    verify = bv.verify_packed2 if protocol == 2 else bv.verify_packed1
    locate = bv.locate_packed2 if protocol == 2 else bv.locate_packed1
    try:
        assert verify(api_classes(base)) is True and locate(api_classes(base)) == []
        assert all(all(single_verdicts(scaled, pk)) for pk in base)
        rnd = random.Random(3)
        pks = [pk.clone() for pk in base]
        PR.mut_a_changed(pks[0], 1, rnd)                        # global 1: only the group equation
        PR.mut_xs_changed(pks[1], 0, rnd)                       # global 2: bit 0
        PR.mut_l_off_curve(pks[1], 2, rnd)                      # global 4: bit 1
        PR.mut_l_replaced_rehashed(pks[3], 1, rnd)              # global 7
        assert verify(api_classes(pks)) is False
        assert locate(api_classes(pks)) == [1, 2, 4, 7]
        singles = [v for pk in pks for v in single_verdicts(scaled, pk)]
        assert singles == [i not in (1, 2, 4, 7) for i in range(8)]
    finally:
        bv.release()


def test_a_flagged_proof_contributes_nothing(gp):
    """Explicit weights: out with a flagged proof present equals out of the call without that proof, the weights of the others kept (a
    wrong a elsewhere keeps both away from the identity)."""
    base = class_list(VALID_SHAPE, 2, False, True, valid=True)
    bv = make_verifier(gp, False)
    try:
        pks = [pk.clone() for pk in base]
        PR.mut_a_changed(pks[3], 0, None)
        PR.mut_xs_changed(pks[1], 1, random.Random(2))          # global index 3: flagged
        ws = explicit_weights(2, 8, 17)
        out, st = mixed_out(gp, bv, 2, pks, PR.pack_weights(ws))
        assert list(st) == [0, 0, 0, 1, 0, 0, 0, 0] and out != bytes(64)
        without = [pks[0], pks[1].subset([0, 2]), pks[2], pks[3]]
        out2, st2 = mixed_out(gp, bv, 2, without, PR.pack_weights(ws[:3] + ws[4:]))
        assert st2 == bytes(7) and out2 == out
    finally:
        bv.release()


# ---- 5. points and argument errors -------------------------------------------------------------------------------------------------------
def raw_call(eng, bv, protocol, arr, n_classes, weights, seed, d_g=None, n_gens=N, out=True, status_len=16):
    out_buf, st_buf = ctypes.create_string_buffer(b"\x55" * 64, 64), ctypes.create_string_buffer(b"\x55" * status_len, status_len)
    rc = eng.lib.bpmi_ipa_verify_batch_packed_mixed_dev(eng.ctx, bv._d[0].ptr if d_g is None else d_g, bv._d[1].ptr, None, n_gens, protocol, n_classes,
                                                        None if arr is None else ctypes.addressof(arr), weights, seed,
                                                        ctypes.cast(out_buf, ctypes.c_void_p) if out else None, ctypes.cast(st_buf, ctypes.c_void_p))
    return rc, eng.lib.bpmi_last_error(eng.ctx).decode(), out_buf.raw, st_buf.raw


def test_only_the_first_n_top_generators_are_checked(gp):
    """validate_points = 2: a non-point at generator index n_top is never read and accepted; one at n_top - 1 is refused, 0xFF.. in out."""
    from bulletproofs_amd.ec import pack_points
    from bulletproofs_amd.engine import packed_class_array
    eng = gp.engine()
    pks = class_list(VALID_SHAPE, 2, False, False, valid=True)          # n_top = 8
    bv = make_verifier(gp, False)
    C = capacity(False)
    arr, keep, total, _, _ = packed_class_array(2, eng_classes(pks))
    d_bad = []
    eng.set_option("validate_points", 2)
    try:
        for index, ok in ((8, True), (7, False)):
            raw = bytearray(pack_points(C.g))
            raw[64 * index + 32] ^= 1
            d_bad.append(eng.upload(bytes(raw)))
            rc, msg, out, st = raw_call(eng, bv, 2, arr, len(pks), None, SEED, d_g=d_bad[-1].ptr)
            if ok:
                assert rc == 0 and out == bytes(64) and st[:total] == bytes(total)
            else:
                assert rc == E_ARG and "d_g[7] is not a point of the curve" in msg and out == b"\xff" * 64
    finally:
        eng.set_option("validate_points", 1)
        for d in d_bad:
            d.free()
        bv.release()
        del keep


def test_argument_errors_write_nothing(gp):
    from bulletproofs_amd import _native
    from bulletproofs_amd.engine import packed_class_array
    eng = gp.engine()
    pks2 = class_list(VALID_SHAPE, 2, False, False, valid=True)
    pks1 = class_list(VALID_SHAPE, 1, False, False, valid=True)
    bv = make_verifier(gp, False)
    try:
        arr2, keep2, total, rec_bytes, pairs = packed_class_array(2, eng_classes(pks2))
        arr1, keep1, _, _, _ = packed_class_array(1, eng_classes(pks1))

        def changed(arr, which, **fields):
            new = (_native.IpaPackedClass * len(arr))()
            ctypes.memmove(new, arr, ctypes.sizeof(arr))
            for name, v in fields.items():
                setattr(new[which], name, v)
            return new
        down = (ctypes.c_uint64 * 4)(5, 4, 4, 4)
        some = ctypes.create_string_buffer(4096)
        cases = [
            (2, arr2, {"n_classes": 0}, "between 1 and 64 classes"),
            (2, arr2, {"n_classes": 65}, "between 1 and 64 classes"),
            (2, None, {}, "between 1 and 64 classes"),
            (3, arr2, {}, "protocol must be 1 or 2"),
            (2, arr2, {"n_gens": 48}, "n_gens must be 2^K, K <= 22"),
            (2, arr2, {"n_gens": 4}, "class 1: k must be at most K"),
            (2, changed(arr2, 1, ab=None), {}, "class 1: null argument"),
            (2, changed(arr2, 3, xs=None), {}, "class 3: null argument (xs and LR may be NULL only at k = 0)"),
            (2, changed(arr2, 0, c=ctypes.addressof(some)), {}, "class 0: c and head must be NULL under protocol 2"),
            (1, changed(arr1, 2, head=None), {}, "class 2: protocol 1 needs c and head"),
            (1, changed(arr1, 1, start=ctypes.addressof(some)), {}, "class 1: start must be NULL under protocol 1"),
            (2, changed(arr2, 1, tr_off=ctypes.addressof(down)), {}, "class 1: tr_off must not decrease"),
            (2, arr2, {"seed": None}, "class 0: weights or a 32-byte seed"),
            (2, changed(arr2, 0, n_proofs=(1 << 16) + 1), {}, "class 0: between 1 and 2^16 proofs per call"),
            (2, arr2, {"d_g": 0}, "null argument"),
            (2, arr2, {"out": False}, "null argument"),
        ]
        for protocol, arr, kw, text in cases:
            n_classes = kw.pop("n_classes", 4)
            seed = kw.pop("seed", SEED)
            rc, msg, out, st = raw_call(eng, bv, protocol, arr, n_classes, None, seed, **kw)
            assert rc == E_ARG and text in msg and "bpmi_ipa_verify_batch_packed_mixed_dev" in msg, (text, rc, msg)
            assert out == b"\x55" * 64 and st == b"\x55" * 16, text
        # the same plan refuses the preparation calls: the records' buffer, the offsets and the status stay as they were
        d = eng.alloc(1 << 16)
        d.upload(b"\x55" * (1 << 16))
        st, offs = ctypes.create_string_buffer(b"\x55" * 16, 16), (ctypes.c_uint64 * 4)(7, 7, 7, 7)
        rc = eng.lib.bpmi_ipa_batch_prepare_mixed_dev(eng.ctx, 2, 2, 4, ctypes.addressof(arr2), None, SEED, d.ptr, ctypes.addressof(offs), d.ptr, d.ptr,
                                                      ctypes.cast(st, ctypes.c_void_p))
        assert rc == E_ARG and "bpmi_ipa_batch_prepare_mixed_dev: class 1: k must be at most K" in eng.lib.bpmi_last_error(eng.ctx).decode()
        assert d.download(1 << 16) == b"\x55" * (1 << 16) and st.raw == b"\x55" * 16 and list(offs) == [7] * 4
        d.free()
        host = ctypes.create_string_buffer(b"\x55" * (1 << 16), 1 << 16)
        hp = ctypes.cast(host, ctypes.c_void_p)
        arr_down = changed(arr2, 1, tr_off=ctypes.addressof(down))
        rc = eng.lib.bpmi_ipa_batch_prepare_mixed(K, 2, 4, ctypes.addressof(arr_down), None, SEED, 1, hp, ctypes.addressof(offs), hp, hp, hp)
        assert rc == E_ARG and "bpmi_ipa_batch_prepare_mixed: class 1: tr_off must not decrease" in eng.lib.bpmi_last_error(None).decode()
        assert host.raw == b"\x55" * (1 << 16) and list(offs) == [7] * 4
        # every class empty: BPMI_OK, the identity, nothing else touched
        empty = (_native.IpaPackedClass * 2)()
        rc, msg, out, st = raw_call(eng, bv, 2, empty, 2, None, SEED)
        assert rc == 0 and out == bytes(64) and st == b"\x55" * 16
        del keep2, keep1
    finally:
        bv.release()


def test_c_program_proves_two_lengths_and_verifies_them_in_one_call(gp, tmp_path):
    """examples/ipa_prove_verify_mixed_c_abi.c: a C99 program over include/bpmi.h and libbpmi.so alone proves with two batch provers of
    n = 8 and n = 64, verifies both classes with one bpmi_ipa_verify_batch_packed_mixed_dev, flips one transcript byte and names the
    proof by its global index."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(repo, "python-bulletproofs_amd")
    exe = str(tmp_path / "ipa_prove_verify_mixed_c_abi")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(repo, "include"),
                           os.path.join(repo, "examples", "ipa_prove_verify_mixed_c_abi.c"), "-o", exe, os.path.join(libdir, "libbpmi.so"),
                           "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"])
    r = subprocess.run([exe, "5", "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "(as proved): VALID, 0 proofs flagged" in r.stdout
    assert "(one transcript byte changed): INVALID, 1 proofs flagged, proof 7 (class 1, its proof 2)" in r.stdout
