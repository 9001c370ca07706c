"""Range proofs of different sizes in one call and ONE MSM on the device: bpmi_rp_batch_verify_mixed_dev through the C ABI and
MixedBatchRangeVerifier on top of it -- the reference-made goldens as mixed batches, equality with the per-class path byte for byte,
weights and verdict indices by the global (class-major) index, rounds and lanes, locate_wire, the argument errors."""
import ctypes
import hashlib
import os
import random
import sys

import pytest

import bulletproofs_amd  # noqa: F401
from bulletproofs_amd import _native
from bulletproofs_amd.rangeproofs import MixedBatchRangeVerifier
from bulletproofs_amd.rangeproofs.batch import BatchRangeVerifier
from bulletproofs_amd.rangeproofs.codec import proof_to_bytes

from helpers import P, Q, gens
from test_batch_verify_cpu import convert_proof, gpt, oracle_decompress, oracle_msm

pytestmark = pytest.mark.gpu
ZERO64 = bytes(64)
E_ARG = -3


@pytest.fixture(scope="module")
def eng():
    from bulletproofs_amd.engine import default_engine
    return default_engine()


@pytest.fixture(scope="module")
def gp():
    import gpu_common
    return gpu_common


def shared_bytes(g, h, u, gs, hs):
    return g.to_le64() + h.to_le64() + u.to_le64() + b"".join(p.to_le64() for p in gs) + b"".join(p.to_le64() for p in hs)


def mixed_call(eng, gens_bytes, N, classes, weights=None, seed=None, n_classes=None, null_class=False):
    """bpmi_rp_batch_verify_mixed_dev as a C caller sees it.  classes: [(n_gens, m, [blobs], commitments as bytes)] ->
    (rc, out, first_bad, message)."""
    keep, arr = [], (_native.RpClass * max(len(classes), 1))()
    npairs = 1
    for c, (n, m, blobs, vb) in enumerate(classes):
        offs = (ctypes.c_uint64 * (len(blobs) + 1))()
        for j, b in enumerate(blobs):
            offs[j + 1] = offs[j] + len(b)
        joined = ctypes.create_string_buffer(b"".join(blobs), max(offs[len(blobs)], 1))
        vbuf = ctypes.create_string_buffer(vb, max(len(vb), 1))
        keep += [offs, joined, vbuf]
        arr[c].n_gens, arr[c].values_per_proof, arr[c].n_proofs = n, m, len(blobs)
        arr[c].blobs, arr[c].blobs_len, arr[c].blob_off, arr[c].v_points = ctypes.addressof(joined), offs[len(blobs)], ctypes.addressof(offs), ctypes.addressof(vbuf)
        npairs += len(blobs) * (m + 6 + 2 * max(n.bit_length() - 1, 0))
    d_gens, d_pts, d_scs = eng.upload(gens_bytes), eng.alloc(64 * npairs), eng.alloc(32 * npairs)
    out = ctypes.create_string_buffer(64)
    bad = ctypes.c_int64(-7)
    try:
        rc = eng.lib.bpmi_rp_batch_verify_mixed_dev(eng.ctx, len(classes) if n_classes is None else n_classes, None if null_class else ctypes.cast(arr, ctypes.c_void_p), N,
                                                    weights, seed, d_gens.ptr, d_pts.ptr, d_scs.ptr, out, ctypes.cast(ctypes.pointer(bad), ctypes.c_void_p))
        return rc, out.raw, bad.value, eng.lib.bpmi_last_error(eng.ctx).decode()
    finally:
        for d in (d_gens, d_pts, d_scs):
            d.free()


def pack(Vs):
    return b"".join(V.to_le64() for V in Vs)


# ---- 1. the reference-made goldens as mixed batches -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def goldens(gp):
    """family -> (g, h, u, gs, hs of the LONGEST proof, [(n_gens, m, commitments, proof object)]): the goldens of a family share (g, h, u)
    and their generator lists are prefixes of one list"""
    from conftest import load_golden
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_wire_golden
    from test_gpu_rangeproofs import inputs
    out = {}
    for family in ("single", "aggregated"):
        cases, lists = [], []
        for c in load_golden("rangeproofs.json")[family]:
            m = c.get("m", 1)
            s, n, gs, hs, g, h, u = inputs(gp, c, m)
            Vs = [gp.to_gpu(P(x)) for x in c["Vs"]] if m > 1 else [gp.to_gpu(P(c["V"]))]
            cases.append((n * m, m, Vs, make_wire_golden.proof_of(c["proof"])))
            lists.append((g, h, u, gs, hs))
        longest = max(lists, key=lambda t: len(t[3]))
        for g, h, u, gs, hs in lists:                # one (g, h, u); every list is the head of the longest
            assert pack([g, h, u]) == pack(longest[:3]) and pack(gs) == pack(longest[3][:len(gs)]) and pack(hs) == pack(longest[4][:len(hs)])
        out[family] = longest + (cases,)
    return out


@pytest.mark.parametrize("family,formats", [("single", (1,) * 7), ("single", (2,) * 7), ("single", (3,) * 7), ("single", (1, 2, 3, 1, 2, 3, 2)), ("aggregated", (1, 2, 3))],
                         ids=["single-v1", "single-v2", "single-v3", "single-mixed-formats", "aggregated"])
def test_goldens_as_one_mixed_batch(eng, goldens, family, formats):
    g, h, u, gs, hs, cases = goldens[family]
    assert len(cases) == len(formats) and sorted(c[0] for c in cases) == ([2, 4, 8, 16, 32, 64, 128] if family == "single" else [64, 128, 512])
    N = len(gs)
    classes = [(n, m, [proof_to_bytes(pr, version=v)], pack(Vs)) for (n, m, Vs, pr), v in zip(cases, formats)]          # classes of ONE proof each
    rc, out, bad, msg = mixed_call(eng, shared_bytes(g, h, u, gs, hs), N, classes, seed=bytes(range(32)))
    assert (rc, out, bad) == (0, ZERO64, -1), msg
    mv = MixedBatchRangeVerifier(g, h, gs, hs, u)
    items = [(Vs if m > 1 else Vs[0], proof_to_bytes(pr, version=v)) for (n, m, Vs, pr), v in zip(cases, formats)]
    assert mv.verify_wire(items) is True and mv.verify_wire(list(reversed(items))) is True
    wrong = list(items)
    wrong[1] = (g if cases[1][1] == 1 else [g] * cases[1][1], wrong[1][1])
    with pytest.raises(Exception, match="^Proof invalid$"):
        mv.verify_wire(wrong)
    mv.release()


# ---- 2 .. 5: classes made by the oracle's prover over the prefixes of one 16-generator list -------------------------------------------------
SHAPES = [(2, 1, 1), (8, 1, 3), (8, 2, 65), (16, 4, 2)]          # (n_gens, m, proofs): the smallest size, two classes over the same generators, an aggregated one


@pytest.fixture(scope="module")
def world():
    from oracle import bp_ref as R
    from oracle import cbind
    gs, hs = gens(16, b"cgs"), gens(16, b"chs")
    g, h, u = (R.elliptic_hash(s) for s in (b"cg", b"ch", b"cu"))
    rnd = random.Random(77)
    classes = []
    for n, m, count in SHAPES:
        bits = n // m
        Vs_all, blobs = [], []
        for j in range(count):
            vs = [R.Zq(rnd.randrange(2 ** bits), Q) for _ in range(m)]
            gammas = [R.mod_hash(b"mx%d-%d-%d-%d" % (n, m, j, t), Q) for t in range(m)]
            Vs_all.append([gpt(R.commitment(g, h, v, ga)) for v, ga in zip(vs, gammas)])
            if m == 1:
                pr = R.range_prove(vs[0], n, g, h, gs[:n], hs[:n], gammas[0], u, seed=b"ms%d-%d" % (n, j), multiexp=cbind.msm)
            else:
                pr = R.aggreg_range_prove(vs, bits, g, h, gs[:n], hs[:n], gammas, u, seed=b"ms%d-%d-%d" % (n, m, j), multiexp=cbind.msm)
            blobs.append(proof_to_bytes(convert_proof(pr)))
            if (n, m, j) == (8, 1, 2):
                other_format = proof_to_bytes(convert_proof(pr), version=2)
        classes.append((n, m, Vs_all, blobs))
    w = dict(g=gpt(g), h=gpt(h), u=gpt(u), gs=[gpt(p) for p in gs], hs=[gpt(p) for p in hs], classes=classes)
    w["class1_proof2_format2"] = other_format
    w["gens_bytes"] = shared_bytes(w["g"], w["h"], w["u"], w["gs"], w["hs"])
    return w


def abi_classes(classes):
    return [(n, m, blobs, pack([V for Vs in Vs_all for V in Vs])) for n, m, Vs_all, blobs in classes]


def with_wrong_commitments(world):
    """one proof in each of two classes with another proof's commitment: every byte-level check passes, the equations do not hold"""
    classes = [(n, m, [list(v) for v in Vs_all], blobs) for n, m, Vs_all, blobs in world["classes"]]
    classes[1][2][2] = list(classes[1][2][0])
    classes[2][2][64] = list(classes[2][2][3])
    assert classes[1][2][2] != world["classes"][1][2][2] and classes[2][2][64] != world["classes"][2][2][64]
    return classes


def test_equal_to_the_per_class_path_byte_for_byte(eng, world):
    classes = with_wrong_commitments(world)
    total = sum(len(c[3]) for c in classes)
    rnd = random.Random(12)
    ws = [rnd.randrange(1, Q) for _ in range(4 * total)]
    weights = b"".join(w.to_bytes(32, "little") for w in ws)
    rc, out, bad, msg = mixed_call(eng, world["gens_bytes"], 16, abi_classes(classes), weights=weights)
    assert (rc, bad) == (0, -1), msg
    assert out != ZERO64                                     # never identity against identity
    # the four single-class calls over the prefixes, each with its slice of the weights
    values, first = [], 0
    for n, m, Vs_all, blobs in classes:
        it = iter(ws[4 * first: 4 * (first + len(blobs))])
        bv = BatchRangeVerifier(world["g"], world["h"], world["gs"][:n], world["hs"][:n], world["u"], rng=lambda: next(it))
        values.append(bv.partial_wire(Vs_all if m > 1 else [v[0] for v in Vs_all], blobs))
        bv.release()
        first += len(blobs)
    assert sum(v != ZERO64 for v in values) == 2
    assert out == eng.ec_sum_bytes(b"".join(values), len(values))
    # the host path through the oracle's MSM with the same weights by global index
    it = iter(ws)
    mv = MixedBatchRangeVerifier(world["g"], world["h"], world["gs"], world["hs"], world["u"], msm=oracle_msm, rng=lambda: next(it), decompress=oracle_decompress)
    items = [(Vs if m > 1 else Vs[0], blob) for n, m, Vs_all, blobs in classes for Vs, blob in zip(Vs_all, blobs)]
    assert [len(idx) for _, _, _, idx in mv.classes(items)] == [c[2] for c in SHAPES]
    assert out == mv.partial_wire(items)
    # and the valid batch is the identity, through the class as well
    rc, ok_out, bad, msg = mixed_call(eng, world["gens_bytes"], 16, abi_classes(world["classes"]), weights=weights)
    assert (rc, ok_out, bad) == (0, ZERO64, -1), msg
    dv = MixedBatchRangeVerifier(world["g"], world["h"], world["gs"], world["hs"], world["u"])
    valid = [(Vs if m > 1 else Vs[0], blob) for n, m, Vs_all, blobs in world["classes"] for Vs, blob in zip(Vs_all, blobs)]
    random.Random(5).shuffle(valid)
    assert dv.verify_wire(valid) is True
    it2 = iter(ws)
    dv2 = MixedBatchRangeVerifier(world["g"], world["h"], world["gs"], world["hs"], world["u"], rng=lambda: next(it2))
    assert dv2.partial_wire(items) == out
    dv.release()
    dv2.release()


def derived_weights(seed, indices):
    out = b""
    for i in indices:
        for t in range(4):
            dg = bytearray(hashlib.sha256(seed + i.to_bytes(8, "little") + bytes([t])).digest())
            dg[31] = 0
            out += bytes(dg)
    return out


def test_weights_follow_the_global_index(eng, world):
    """Two classes of the same shape, each holding the SAME valid proof, with commitments V + D and V - D.  Under equal weights the two
    errors cancel (unit weights: the identity -- this documents the construction); under weights by the GLOBAL index they do not, and
    a class that restarted its weight index at 0 would give both proofs the weights of index 0 and return the identity."""
    from oracle.ec import Point, secp256k1
    n, m, Vs_all, blobs = world["classes"][1]
    V = Point(Vs_all[0][0].x, Vs_all[0][0].y, secp256k1)
    D = secp256k1.G * 5
    plus, minus = gpt(V + D), gpt(V - D)
    classes = [(n, m, [blobs[0]], plus.to_le64()), (n, m, [blobs[0]], minus.to_le64())]
    unit = (1).to_bytes(32, "little") * 8
    rc, out, bad, msg = mixed_call(eng, world["gens_bytes"], 16, classes, weights=unit)
    assert (rc, out, bad) == (0, ZERO64, -1), msg
    seed = hashlib.sha256(b"mixed seed").digest()
    rc, by_seed, bad, msg = mixed_call(eng, world["gens_bytes"], 16, classes, seed=seed)
    assert (rc, bad) == (0, -1) and by_seed != ZERO64, msg
    rc, explicit, bad, msg = mixed_call(eng, world["gens_bytes"], 16, classes, weights=derived_weights(seed, (0, 1)))
    assert (rc, bad) == (0, -1) and explicit == by_seed, msg
    rc, restarted, bad, msg = mixed_call(eng, world["gens_bytes"], 16, classes, weights=derived_weights(seed, (0, 0)))
    assert (rc, restarted, bad) == (0, ZERO64, -1), msg              # what a per-class index would compute


def test_first_bad_is_global_and_smallest(eng, world):
    base = [0, 1, 4, 69]
    classes = abi_classes(world["classes"])

    def flipped(blob, pos):
        b = bytearray(blob)
        b[pos] ^= 1
        return bytes(b)

    # a byte of the last transcript (the Protocol-2 hash chain no longer spells its challenge): proof 1 of class 2 and proof 0 of class 3
    mutated = [list(c) for c in classes]
    mutated[2][2] = list(mutated[2][2])
    mutated[3][2] = list(mutated[3][2])
    mutated[2][2][1] = flipped(mutated[2][2][1], len(mutated[2][2][1]) - 3)
    mutated[3][2][0] = flipped(mutated[3][2][0], len(mutated[3][2][0]) - 3)
    seed = b"\x21" * 32
    rc, out, bad, msg = mixed_call(eng, world["gens_bytes"], 16, [tuple(c) for c in mutated], seed=seed)
    assert (rc, bad) == (0, base[2] + 1), msg
    rc, out, bad, msg = mixed_call(eng, world["gens_bytes"], 16, [tuple(c) for c in mutated[:2]] + [classes[2], tuple(mutated[3])], seed=seed)
    assert (rc, bad) == (0, base[3]), msg
    # t_hat (the 32 bytes at offset 70 of a format-1 proof) is in no transcript: a flipped byte of it, still below q, passes every byte-level
    # check and fails the equations -- no index, a value that is not the identity
    that = [list(c) for c in classes]
    that[2][2] = list(that[2][2])
    that[2][2][1] = flipped(that[2][2][1], 70 + 31)
    rc, out, bad, msg = mixed_call(eng, world["gens_bytes"], 16, [tuple(c) for c in that], seed=seed)
    assert (rc, bad) == (0, -1) and out != ZERO64, msg
    # a bad point encoding (an x with no point on the curve, or a bad prefix) in class 0 alone: its index
    n0, m0, blobs0, vb0 = classes[0]
    comp = 6 + 32 * (5 + 1)                                  # the first compressed point of a k = 1 proof
    for x in range(1, 40):
        cand = bytearray(blobs0[0])
        cand[comp + 32] ^= x
        pts, ok = eng.ec_decompress_batch_bytes(bytes(cand[comp: comp + 33]), 1)
        if 0 in bytes(ok):
            break
    else:
        raise AssertionError("no invalid encoding found")
    rc, out, bad, msg = mixed_call(eng, world["gens_bytes"], 16, [(n0, m0, [bytes(cand)], vb0)] + classes[1:], seed=seed)
    assert (rc, bad) == (0, 0), msg
    mv = MixedBatchRangeVerifier(world["g"], world["h"], world["gs"], world["hs"], world["u"])
    items = [(Vs if m > 1 else Vs[0], blob) for n, m, Vs_all, blobs in world["classes"] for Vs, blob in zip(Vs_all, blobs)]
    items[base[2] + 1] = (items[base[2] + 1][0], mutated[2][2][1])
    with pytest.raises(Exception, match="^Proof invalid$"):
        mv.partial_wire(items)
    mv.release()
    # a format-2 proof inside a format-1 class: the argument error, naming the class
    n1, m1, blobs1, vb1 = classes[1]
    v2 = world["class1_proof2_format2"]
    rc, out, bad, msg = mixed_call(eng, world["gens_bytes"], 16, [classes[0], (n1, m1, blobs1[:2] + [v2], vb1)] + classes[2:], seed=seed)
    assert rc == E_ARG and "mixed wire formats: class 1, proof 2 is format 2 in a format-1 batch" in msg and out == b"\xff" * 64


@pytest.mark.parametrize("lanes", [1, 16])
def test_rounds_and_lanes_give_the_same_bytes(eng, world, lanes):
    classes = abi_classes(with_wrong_commitments(world))
    total = sum(len(c[2]) for c in classes)
    rnd = random.Random(12)
    weights = b"".join(rnd.randrange(1, Q).to_bytes(32, "little") for _ in range(4 * total))
    rc, want, bad, msg = mixed_call(eng, world["gens_bytes"], 16, classes, weights=weights)
    assert (rc, bad) == (0, -1) and want != ZERO64, msg
    try:
        eng.set_option("rp_rows", 2)
        eng.set_option("rp_lanes", lanes)
        rc, got, bad, msg = mixed_call(eng, world["gens_bytes"], 16, classes, weights=weights)
    finally:
        eng.set_option("rp_rows", 0)
        eng.set_option("rp_lanes", 0)
    assert (rc, bad) == (0, -1) and got == want, msg


def test_locate_wire_in_the_callers_order(eng, world):
    mv = MixedBatchRangeVerifier(world["g"], world["h"], world["gs"], world["hs"], world["u"])
    items = [(Vs if m > 1 else Vs[0], blob) for n, m, Vs_all, blobs in world["classes"] for Vs, blob in zip(Vs_all, blobs)]
    order = list(range(len(items)))
    random.Random(8).shuffle(order)
    shuffled = [items[i] for i in order]
    assert mv.locate_wire(shuffled) == []
    # three invalid proofs in two classes: a wrong commitment and a flipped byte in class (8, 2), a wrong commitment in class (8, 1)
    bad_orig = {2: (items[1][0], items[2][1]), 10: (items[11][0], items[10][1]), 40: (items[40][0], items[40][1][:-3] + bytes([items[40][1][-3] ^ 4]) + items[40][1][-2:])}
    for i, it in bad_orig.items():
        items[i] = it
    shuffled = [items[i] for i in order]
    assert mv.locate_wire(shuffled) == sorted(order.index(i) for i in bad_orig)
    mv.release()


# ---- 7. argument errors through the C ABI ----------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_ctx_usable(eng, world):
    classes = abi_classes(world["classes"])
    gb, seed = world["gens_bytes"], b"\x05" * 32
    n1, m1, blobs1, vb1 = classes[1]
    cases = [
        (dict(classes=classes[:1], n_classes=0), "n_classes must be in [1, 64]"),
        (dict(classes=classes[:1], n_classes=65), "n_classes must be in [1, 64]"),
        (dict(classes=classes, N=8), "class 3: n_gens exceeds n_gens_max"),
        (dict(classes=classes, null_class=True), "null argument"),
        (dict(classes=[classes[0], (n1, m1, [], b"")]), "class 1: n_proofs must be in [1, 2^22]"),
    ]
    for kw, text in cases:
        N = kw.pop("N", 16)
        rc, out, bad, msg = mixed_call(eng, gb, N, kw.pop("classes"), seed=seed, **kw)
        assert rc == E_ARG and text in msg and bad == -7, (text, msg)          # (nothing written before the plan has decided)
        rc, out, bad, msg = mixed_call(eng, gb, 16, classes, seed=seed)                   # the ctx is usable: a valid call succeeds
        assert (rc, out, bad) == (0, ZERO64, -1), msg
