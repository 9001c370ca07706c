"""Which groups of a MIXED batch of range proofs hold an invalid one, in one native call: bpmi_rp_batch_group_values_mixed_dev through the
C ABI and MixedBatchRangeVerifier.group_values_packed / group_values_wire / locate_wire(group=None) on top of it -- equality with the
single-class group call byte for byte (light, mid and msm_run routes; a class over the whole generator list beside shorter prefixes),
the sum of the values against the mixed verify call, faults by class-major index, the preparation options, the argument errors."""
import ctypes
import random

import pytest

import bulletproofs_amd  # noqa: F401
from bulletproofs_amd import _native
from bulletproofs_amd.rangeproofs import MixedBatchRangeVerifier
from bulletproofs_amd.rangeproofs.batch import BatchRangeVerifier
from bulletproofs_amd.rangeproofs.codec import proof_to_bytes

from helpers import Q, gens
from test_batch_verify_cpu import convert_proof, gpt

pytestmark = pytest.mark.gpu
ZERO64 = bytes(64)
FF64 = b"\xff" * 64
E_ARG = -3
FILL = 0xA5                                                      # what the output buffers hold before a call
SHAPES = [(2, 1, 1), (8, 1, 3), (8, 2, 65), (16, 4, 2)]          # (n_gens, m, proofs): two classes over the same generators, one over the whole list
FIRST = [0, 1, 4, 69]                                            # global index of every class's proof 0
TOTAL = 71


@pytest.fixture(scope="module")
def eng():
    from bulletproofs_amd.engine import default_engine
    return default_engine()


def pack(Vs):
    return b"".join(V.to_le64() for V in Vs)


@pytest.fixture(scope="module")
def world():
    """Classes made by the oracle's prover over the prefixes of one 16-generator list."""
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
    w["gens_bytes"] = pack([w["g"], w["h"], w["u"]] + w["gs"] + w["hs"])
    rnd = random.Random(12)
    w["ws"] = [rnd.randrange(1, Q) for _ in range(4 * 10 * TOTAL)]           # explicit weights, enough for the repeated class too
    return w


def wbytes(ws):
    return b"".join(w.to_bytes(32, "little") for w in ws)


def with_wrong_commitments(world):
    """one proof in each of two classes with another proof's commitment: every byte-level check passes, the equations do not hold"""
    classes = [(n, m, [list(v) for v in Vs_all], list(blobs)) for n, m, Vs_all, blobs in world["classes"]]
    classes[1][2][2] = list(classes[1][2][0])
    classes[2][2][64] = list(classes[2][2][3])
    return classes


def fill_classes(classes):
    keep, arr = [], (_native.RpClass * max(len(classes), 1))()
    npairs = 1
    for c, (n, m, Vs_all, blobs) in enumerate(classes):
        vb = pack([V for Vs in Vs_all for V in Vs])
        offs = (ctypes.c_uint64 * (len(blobs) + 1))()
        for j, b in enumerate(blobs):
            offs[j + 1] = offs[j] + len(b)
        joined = ctypes.create_string_buffer(b"".join(blobs), max(offs[len(blobs)], 1))
        vbuf = ctypes.create_string_buffer(vb, max(len(vb), 1))
        keep += [offs, joined, vbuf]
        arr[c].n_gens, arr[c].values_per_proof, arr[c].n_proofs = n, m, len(blobs)
        arr[c].blobs, arr[c].blobs_len, arr[c].blob_off, arr[c].v_points = ctypes.addressof(joined), offs[len(blobs)], ctypes.addressof(offs), ctypes.addressof(vbuf)
        npairs += len(blobs) * (m + 6 + 2 * max(n.bit_length() - 1, 0))
    return keep, arr, npairs


def group_call(eng, world, classes, groups, weights=None, seed=None, N=16, n_classes=None, null=(), gens_bytes=None):
    """bpmi_rp_batch_group_values_mixed_dev as a C caller sees it.  classes: [(n_gens, m, [[V ..] per proof], [blobs])] ->
    (rc, [values], [value_off], status, message); the raw output buffers, filled with FILL before the call, are in the last element."""
    keep, arr, npairs = fill_classes(classes)
    total = sum(len(c[3]) for c in classes)
    ngroups = sum(-(-len(c[3]) // max(1, min(g, len(c[3])))) if len(c[3]) else 0 for c, g in zip(classes, groups))
    grp = (ctypes.c_uint64 * max(len(groups), 1))(*groups)
    values = ctypes.create_string_buffer(bytes([FILL]) * (64 * ngroups + 64), 64 * ngroups + 64)
    status = ctypes.create_string_buffer(bytes([FILL]) * (total + 8), total + 8)
    value_off = (ctypes.c_uint64 * (len(classes) + 2))(*([FILL] * (len(classes) + 2)))
    d_gens, d_pts, d_scs = eng.upload(gens_bytes or world["gens_bytes"]), eng.alloc(64 * npairs), eng.alloc(32 * npairs)
    ptr = lambda name, buf: None if name in null else ctypes.cast(buf, ctypes.c_void_p)
    try:
        rc = eng.lib.bpmi_rp_batch_group_values_mixed_dev(eng.ctx, len(classes) if n_classes is None else n_classes, ptr("classes", arr), N, ptr("group", grp), weights, seed,
                                                          None if "d_gens" in null else d_gens.ptr, d_pts.ptr, d_scs.ptr, ptr("values", values), ptr("value_off", value_off),
                                                          ptr("status", status))
        msg = eng.lib.bpmi_last_error(eng.ctx).decode()
    finally:
        for d in (d_gens, d_pts, d_scs):
            d.free()
    del keep
    raw = values.raw
    return rc, [raw[64 * t: 64 * t + 64] for t in range(ngroups)], list(value_off)[:len(classes) + 1], status.raw[:total], msg, (raw, status.raw, list(value_off))


def single_class(world, cls, group, ws):
    """bpmi_rp_batch_group_values_dev over the class's prefix generators under its slice of the weights: (values, status)"""
    n, m, Vs_all, blobs = cls
    it = iter(ws)
    bv = BatchRangeVerifier(world["g"], world["h"], world["gs"][:n], world["hs"][:n], world["u"], rng=lambda: next(it))
    try:
        return bv.group_values_wire(Vs_all if m > 1 else [v[0] for v in Vs_all], blobs, group=group)
    finally:
        bv.release()


def expected(world, classes, groups, ws):
    values, status, value_off, first = [], b"", [0], 0
    for cls, g in zip(classes, groups):
        v, st = single_class(world, cls, g, ws[4 * first: 4 * (first + len(cls[3]))])
        values += v
        status += st
        value_off.append(len(values))
        first += len(cls[3])
    return values, value_off, status


def mixed_out(eng, world, classes, weights):
    keep, arr, npairs = fill_classes(classes)
    d_gens, d_pts, d_scs = eng.upload(world["gens_bytes"]), eng.alloc(64 * npairs), eng.alloc(32 * npairs)
    out, bad = ctypes.create_string_buffer(64), ctypes.c_int64(-7)
    try:
        rc = eng.lib.bpmi_rp_batch_verify_mixed_dev(eng.ctx, len(classes), ctypes.cast(arr, ctypes.c_void_p), 16, weights, None, d_gens.ptr, d_pts.ptr, d_scs.ptr, out,
                                                    ctypes.cast(ctypes.pointer(bad), ctypes.c_void_p))
    finally:
        for d in (d_gens, d_pts, d_scs):
            d.free()
    del keep
    assert (rc, bad.value) == (0, -1)
    return out.raw


# [1, 2, 8, 2]: every class light; [1, 3, 64, 2]: class 2 has 19 + 64 x 14 = 915 pairs and runs mid beside light launches; a group above
# every class's size; one proof per group.  Classes 1 and 2 share n_gens = 8 with different m; class 3 has n_c = 16 = N and reads the
# generator list itself beside the copies for n_c = 2 and 8 (whose hs start at another offset).
@pytest.mark.parametrize("groups", [[1, 2, 8, 2], [1, 3, 64, 2], [5, 10, 100, 7], [1, 1, 1, 1]], ids=["light", "mid-beside-light", "above-class-size", "ones"])
def test_equal_to_the_single_class_call_and_sums_to_the_mixed_value(eng, world, groups):
    ws = world["ws"][:4 * TOTAL]
    for classes in (with_wrong_commitments(world), world["classes"]):
        rc, values, value_off, status, msg, _ = group_call(eng, world, classes, groups, weights=wbytes(ws))
        assert rc == 0, msg
        want_values, want_off, want_status = expected(world, classes, groups, ws)
        assert value_off == want_off and status == want_status == bytes(TOTAL)
        assert values == want_values
        out = mixed_out(eng, world, classes, wbytes(ws))
        assert eng.ec_sum_bytes(b"".join(values), len(values)) == out
        if classes is world["classes"]:
            assert out == ZERO64 and all(v == ZERO64 for v in values)
        else:
            # a wrong commitment: exactly one non-identity value per fault, in its own group, status 0
            hit = [t for t, v in enumerate(values) if v != ZERO64]
            g1, g2 = min(groups[1], 3), min(groups[2], 65)
            assert hit == [value_off[1] + 2 // g1, value_off[2] + 64 // g2] and out != ZERO64


def test_the_msm_run_route_gives_the_single_class_bytes(eng, world):
    """class (8, 2) with its 65 proofs ten times over and group = 640: 19 + 640 x 14 = 8 979 pairs, above the one-launch kernel's 8 448 --
    its first group runs as an MSM of its own, its last (10 proofs) too, beside a light class and a class over the whole list"""
    n, m, Vs_all, blobs = with_wrong_commitments(world)[2]
    classes = [world["classes"][0], (n, m, Vs_all * 10, blobs * 10), world["classes"][3]]
    groups = [1, 640, 1]
    total = 1 + 650 + 2
    ws = world["ws"][:4 * total]
    rc, values, value_off, status, msg, _ = group_call(eng, world, classes, groups, weights=wbytes(ws))
    assert rc == 0, msg
    want_values, want_off, want_status = expected(world, classes, groups, ws)
    assert value_off == want_off == [0, 1, 3, 5] and status == want_status == bytes(total)
    assert values == want_values
    assert values[1] != ZERO64 and values[2] != ZERO64 and values[0] == values[3] == values[4] == ZERO64          # proof 64 + 65 j is wrong: both groups hold some


def flipped(blob, pos, x=1):
    b = bytearray(blob)
    b[pos] ^= x
    return bytes(b)


def invalid_encoding(eng, blob, k):
    """blob with the x coordinate of its first compressed point replaced by one that is on no curve point"""
    comp = 6 + 32 * (5 + k)
    for x in range(1, 40):
        cand = flipped(blob, comp + 32, x)
        pts, ok = eng.ec_decompress_batch_bytes(cand[comp: comp + 33], 1)
        if 0 in bytes(ok):
            return cand
    raise AssertionError("no invalid encoding found")


@pytest.mark.parametrize("fault,bit", [("transcript", 1), ("point", 2)])
def test_a_flagged_proof_takes_part_in_no_group(eng, world, fault, bit):
    """Class 1 (three proofs, one group of 3, a wrong commitment at its proof 0 so that the group's value is not the identity): its LAST
    proof is flagged, so the group's value must be that of the class with two proofs, under the weights of the same global indices."""
    classes = [(n, m, [list(v) for v in Vs_all], list(blobs)) for n, m, Vs_all, blobs in world["classes"]]
    classes[1][2][0] = list(classes[1][2][1])
    blob = classes[1][3][2]
    classes[1][3][2] = flipped(blob, len(blob) - 3) if fault == "transcript" else invalid_encoding(eng, blob, 3)
    groups = [1, 3, 8, 2]
    ws = world["ws"][:4 * TOTAL]
    rc, values, value_off, status, msg, _ = group_call(eng, world, classes, groups, weights=wbytes(ws))
    assert rc == 0, msg
    bad = FIRST[1] + 2
    # class-major index; in wire format 1 the encodings are part of a transcript, so a changed one may fail a byte-level check as well
    assert [i for i in range(TOTAL) if status[i]] == [bad] and status[bad] & bit and (fault == "point" or status[bad] == 1)
    without = [classes[0], (8, 1, classes[1][2][:2], classes[1][3][:2])] + classes[2:]
    rc, ref, ref_off, ref_status, msg, _ = group_call(eng, world, without, groups, weights=wbytes(ws[:4 * bad] + ws[4 * (bad + 1):]))
    assert rc == 0 and ref_status == bytes(TOTAL - 1), msg
    assert value_off == ref_off and values == ref
    assert [t for t, v in enumerate(values) if v != ZERO64] == [value_off[1]]               # the wrong commitment's group, and no other


def test_a_proof_of_another_format_is_the_argument_error_naming_the_class(eng, world):
    classes = [(n, m, Vs_all, list(blobs)) for n, m, Vs_all, blobs in world["classes"]]
    classes[1][3][2] = world["class1_proof2_format2"]
    rc, values, value_off, status, msg, _ = group_call(eng, world, classes, [1, 2, 8, 2], seed=b"\x21" * 32)
    assert rc == E_ARG and "mixed wire formats: class 1, proof 2 is format 2 in a format-1 batch" in msg
    assert all(v == FF64 for v in values)


def test_a_profiling_run_of_one_role_flags_every_proof(eng, world):
    try:
        eng.set_option("rp_only_role", 0)
        rc, values, value_off, status, msg, _ = group_call(eng, world, world["classes"], [1, 2, 8, 2], seed=b"\x09" * 32)
    finally:
        eng.set_option("rp_only_role", -1)
    assert rc == 0 and len(status) == TOTAL and all(status), msg
    assert values == [ZERO64] * 13                       # no proof takes part in a group


class RawPoint:
    """64 bytes standing where a commitment stands"""
    def __init__(self, raw):
        self.raw = raw

    def to_le64(self):
        return self.raw


def test_a_call_refused_for_a_point_leaves_ff_in_every_value(eng, world):
    """a commitment that is not a point of the curve is refused with its index among the call's commitments, class-major; from validation
    level 2 so is a generator"""
    off_curve = (1).to_bytes(32, "little") * 2                                # (1, 1): 1 != 1 + 7
    classes = [(n, m, [list(v) for v in Vs_all], blobs) for n, m, Vs_all, blobs in world["classes"]]
    classes[2][2][5][1] = RawPoint(off_curve)                                 # commitment 1 + 3 + 2 x 5 + 1 of the call
    groups, seed = [1, 2, 8, 2], b"\x07" * 32
    text = "bpmi_rp_batch_group_values_mixed_dev: %s is not a point of the curve"
    rc, values, value_off, status, msg, _ = group_call(eng, world, classes, groups, seed=seed)
    assert (rc, msg) == (E_ARG, text % "v_points[15]") and values == [FF64] * 13
    gb = world["gens_bytes"]
    try:
        eng.set_option("validate_points", 2)
        rc, values, value_off, status, msg, _ = group_call(eng, world, world["classes"], groups, seed=seed, gens_bytes=gb[: 64 * 5] + off_curve + gb[64 * 6:])
        assert (rc, msg) == (E_ARG, text % "d_gens[5]") and values == [FF64] * 13
        rc, values, value_off, status, msg, _ = group_call(eng, world, world["classes"], groups, seed=seed)
        assert rc == 0 and values == [ZERO64] * 13 and status == bytes(TOTAL), msg
    finally:
        eng.set_option("validate_points", 1)


@pytest.mark.parametrize("option,value", [("rp_rows", 25), ("rp_lanes", 16), ("rp_overlap", 0)])
def test_the_preparation_options_give_the_same_bytes(eng, world, option, value):
    """rp_rows = 25: the class of 65 proofs runs in three rounds, groups of 8 straddle them; rp_overlap = 0: the decoding in front of the rounds"""
    classes = with_wrong_commitments(world)
    classes[2][3][9] = invalid_encoding(eng, classes[2][3][9], 3)                      # a point flag the verdicts must see in every order of the stages
    classes[2][3][30] = flipped(classes[2][3][30], len(classes[2][3][30]) - 3)
    groups, weights = [1, 2, 8, 2], wbytes(world["ws"][:4 * TOTAL])
    rc, want, want_off, want_status, msg, _ = group_call(eng, world, classes, groups, weights=weights)
    assert rc == 0 and want_status[FIRST[2] + 9] & 2 and want_status[FIRST[2] + 30] == 1 and sum(1 for s in want_status if s) == 2, msg
    default = 1 if option == "rp_overlap" else 0
    try:
        eng.set_option(option, value)
        rc, got, got_off, got_status, msg, _ = group_call(eng, world, classes, groups, weights=weights)
    finally:
        eng.set_option(option, default)
    assert rc == 0 and (got, got_off, got_status) == (want, want_off, want_status), msg


def test_locate_wire_by_groups_equals_the_class_by_class_path(eng, world):
    mv = MixedBatchRangeVerifier(world["g"], world["h"], world["gs"], world["hs"], world["u"])
    items = [(Vs if m > 1 else Vs[0], blob) for n, m, Vs_all, blobs in world["classes"] for Vs, blob in zip(Vs_all, blobs)]
    order = list(range(len(items)))
    random.Random(8).shuffle(order)
    try:
        shuffled = [items[i] for i in order]
        assert mv.locate_wire(shuffled, group=None) == mv.locate_wire(shuffled) == []
        values, value_off, status, index_lists = mv.group_values_wire(shuffled)
        assert value_off == [0, 1, 2, 3, 4] and values == [ZERO64] * 4 and status == bytes(TOTAL)
        assert [len(x) for x in index_lists] == [1, 3, 65, 2] and sorted(i for x in index_lists for i in x) == list(range(TOTAL))
        # one wrong commitment: at level 2 only class (8, 2) has a selection, the other three are left out of the call
        one = list(items)
        one[10] = (items[11][0], items[10][1])
        shuffled = [one[i] for i in order]
        assert mv.locate_wire(shuffled, group=None) == mv.locate_wire(shuffled) == [order.index(10)]
        # several across classes -- wrong commitments in (8, 1) and (8, 2), a flipped byte, an invalid point in (16, 4) -- and one unreadable item
        many = list(items)
        many[2] = (items[1][0], items[2][1])
        many[10] = (items[11][0], items[10][1])
        many[40] = (items[40][0], flipped(items[40][1], len(items[40][1]) - 3, 4))
        many[70] = (items[70][0], invalid_encoding(eng, items[70][1], 4))
        many[20] = (items[20][0], b"BPRP1")
        shuffled = [many[i] for i in order]
        want = sorted(order.index(i) for i in (2, 10, 20, 40, 70))
        assert mv.locate_wire(shuffled) == want
        assert mv.locate_wire(shuffled, group=None) == want
        assert mv.locate_wire(shuffled, group=4) == want and mv.locate_wire(shuffled, group=[1, 2, 16, 1]) == want
    finally:
        mv.release()


def test_argument_errors_leave_the_ctx_usable_and_the_outputs_untouched(eng, world):
    classes = world["classes"]
    n1, m1 = classes[1][0], classes[1][1]
    groups, seed = [1, 2, 8, 2], b"\x05" * 32
    cases = [
        (dict(null=("group",)), "null argument (group)"),
        (dict(null=("values",)), "null argument (values, value_off and status)"),
        (dict(null=("value_off",)), "null argument (values, value_off and status)"),
        (dict(null=("status",)), "null argument (values, value_off and status)"),
        (dict(null=("classes",)), "null argument"),
        (dict(null=("d_gens",)), "null argument"),
        (dict(groups=[1, 2, 0, 2]), "class 2: group must be at least 1"),
        (dict(n_classes=0), "n_classes must be in [1, 64]"),
        (dict(N=8), "class 3: n_gens exceeds n_gens_max"),
        (dict(classes=[classes[0], (n1, m1, [], [])], groups=[1, 1]), "class 1: n_proofs must be in [1, 2^22]"),
    ]
    for kw, text in cases:
        kw = dict(kw)
        rc, values, value_off, status, msg, (raw_v, raw_st, raw_off) = group_call(eng, world, kw.pop("classes", classes), kw.pop("groups", groups), seed=seed, **kw)
        assert rc == E_ARG and text in msg, (text, msg)
        assert set(raw_v) == {FILL} and set(raw_st) == {FILL} and set(raw_off) == {FILL}, text             # (nothing written before the plan has decided)
        rc, values, value_off, status, msg, _ = group_call(eng, world, classes, groups, seed=seed)           # the ctx is usable: a valid call succeeds
        assert rc == 0 and values == [ZERO64] * 13 and value_off == [0, 1, 3, 12, 13] and status == bytes(TOTAL), msg
