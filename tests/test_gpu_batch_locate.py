"""Naming the invalid proofs of a rejected batch on the GPU (bpmi_rp_batch_group_values_dev: per-proof verdict bytes, per-group
column sums, all groups' MSMs in one launch; BatchRangeVerifier.group_values_wire / locate_wire).  The yardsticks are the paths that
existed before: partial_wire of a group's sub-batch with that group's slice of the same weights (byte for byte), and the host
preparation with the oracle's MSM, one proof at a time."""
import ctypes
import random

import pytest

import bulletproofs_amd  # noqa: F401
from bulletproofs_amd.ec import secp256k1
from bulletproofs_amd.engine import EngineError
from bulletproofs_amd.rangeproofs.batch import BatchRangeVerifier
from bulletproofs_amd.rangeproofs.codec import proof_to_bytes

from helpers import Q
from test_batch_verify_cpu import make_batch, oracle_msm
from test_gpu_batch_dev import _v2, _v3, dev_prepare, offsets_of

pytestmark = pytest.mark.gpu

ZERO = bytes(64)
K = 3                                   # n = 8
PTS_AT = 6 + 32 * (5 + K)               # the 6 + 2k compressed points of a wire proof (all formats)


@pytest.fixture(scope="module")
def eng():
    from bulletproofs_amd.engine import default_engine
    return default_engine()


@pytest.fixture(scope="module")
def batch():
    """12 valid 8-bit proofs with their commitments, in the three wire formats (made once, never changed)."""
    b = make_batch(12, n=8)
    b["v1"] = [proof_to_bytes(pr) for pr in b["proofs"]]
    b["v2"] = _v2(b["proofs"])
    b["v3"] = _v3(b["proofs"])
    return b


def verifier(b, ws=None):
    if ws is None:
        return BatchRangeVerifier(b["g"], b["h"], b["gs"], b["hs"], b["u"])
    it = iter(ws)
    return BatchRangeVerifier(b["g"], b["h"], b["gs"], b["hs"], b["u"], rng=lambda: next(it))


def weights_for(count, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(1, Q) for _ in range(4 * count)]


def group_values(b, Vs, blobs, ws, group, **kw):
    bv = verifier(b, ws)
    try:
        return bv.group_values_wire(Vs, blobs, group=group, **kw)
    finally:
        bv.release()


def expected_values(b, Vs, blobs, ws, group, skip=()):
    """partial_wire of every group's sub-batch without the proofs in `skip`; every proof keeps its own four weights."""
    out = []
    for lo in range(0, len(blobs), group):
        idx = [i for i in range(lo, min(lo + group, len(blobs))) if i not in skip]
        if not idx:
            out.append(ZERO)
            continue
        bv = verifier(b, [w for i in idx for w in ws[4 * i: 4 * i + 4]])
        try:
            out.append(bv.partial_wire([Vs[i] for i in idx], [blobs[i] for i in idx]))
        finally:
            bv.release()
    return out


def flip_transcript_byte(blob):
    """Format 1: a digit inside the Protocol-2 transcript.  Formats 2 and 3 carry no transcripts: the last byte of the Protocol-1 seed,
    from which the device rebuilds them -- the challenge the proof claims is no longer their hash."""
    bad = bytearray(blob)
    if blob[4:5] == b"1":
        bad[-3] ^= 1
    else:
        bad[len(bad) - 1 - (32 * (6 + 2 * K) if blob[4:5] == b"3" else 0)] ^= 1
    return bytes(bad)


def off_curve_point(blob, t=2):
    """Point t of the proof replaced by an encoding whose x is on no point of the curve."""
    p = secp256k1.p
    bad = bytearray(blob)
    at = PTS_AT + 33 * t + 1
    x = int.from_bytes(bad[at: at + 32], "big")
    while True:
        x = (x + 1) % p
        if pow((x * x * x + 7) % p, (p - 1) // 2, p) != 1:
            break
    bad[at: at + 32] = x.to_bytes(32, "big")
    return bytes(bad)


def wrong_y(blob_v3, t=5):
    """Format 3: the y coordinate of point t is another number below p."""
    npts = 6 + 2 * K
    bad = bytearray(blob_v3)
    at = len(bad) - 32 * npts + 32 * t
    y = int.from_bytes(bad[at: at + 32], "big")
    bad[at: at + 32] = ((y + 1) % secp256k1.p).to_bytes(32, "big")
    return bytes(bad)


def t_hat_plus_one(blob):
    bad = bytearray(blob)
    t_hat = int.from_bytes(bad[70:102], "big")
    bad[70:102] = ((t_hat + 1) % Q).to_bytes(32, "big")
    return bytes(bad)


@pytest.mark.parametrize("group", [1, 4, 9, 16])
def test_group_values_equal_partial_wire_of_the_sub_batches(batch, group):
    """9 proofs, fixed weights, one wrong commitment: values[t] is partial_wire of group t's sub-batch with its slice of the weights,
    byte for byte; only the wrong proof's group is not the identity; no proof is flagged."""
    Vs, blobs = list(batch["Vs"][:9]), batch["v1"][:9]
    Vs[5] = batch["Vs"][6]
    ws = weights_for(9, 41)
    values, status = group_values(batch, Vs, blobs, ws, group)
    g = min(group, 9)
    assert len(values) == (9 + g - 1) // g and status == bytes(9)
    assert values == expected_values(batch, Vs, blobs, ws, g)
    assert [t for t, v in enumerate(values) if v != ZERO] == [5 // g]


@pytest.mark.parametrize("fmt", ["v1", "v3"])
def test_flagged_proofs_drop_out_of_their_groups(batch, fmt):
    """One proof with a flipped transcript byte (format 3: a flipped seed byte) and one with an invalid point encoding (format 3:
    a wrong y) in one batch: their status bits say which check failed, their groups' values are those of the groups without them --
    here the identity, the rest is valid -- and with a wrong commitment elsewhere in the group, partial_wire of the group without them."""
    Vs, blobs = list(batch["Vs"][:9]), list(batch[fmt][:9])
    blobs[2] = flip_transcript_byte(blobs[2])
    blobs[6] = off_curve_point(blobs[6]) if fmt == "v1" else wrong_y(blobs[6])
    ws = weights_for(9, 43)
    values, status = group_values(batch, Vs, blobs, ws, 4)
    assert status[2] == 1 and status[6] & 2 and (fmt == "v1" or status[6] == 2)
    assert [i for i in range(9) if status[i]] == [2, 6]
    assert values == [ZERO, ZERO, ZERO]
    Vs[3], Vs[4] = batch["Vs"][4], batch["Vs"][3]        # proofs 3 (group 0) and 4 (group 1) now fail their equations
    values, status = group_values(batch, Vs, blobs, ws, 4)
    assert [i for i in range(9) if status[i]] == [2, 6]
    assert values == expected_values(batch, Vs, blobs, ws, 4, skip=(2, 6))
    assert values[0] != ZERO and values[1] != ZERO and values[2] == ZERO
    # a whole group of flagged proofs is the identity
    values, status = group_values(batch, [batch["Vs"][0]] * 2, [blobs[2], blobs[6]], weights_for(2, 44), 2)
    assert values == [ZERO] and status[0] == 1 and status[1] & 2


def rejected_one_by_one(b, Vs, blobs):
    """The proofs the host path rejects when each is verified alone: host preparation, the oracle's MSM."""
    out = []
    for i, (V, blob) in enumerate(zip(Vs, blobs)):
        bv = BatchRangeVerifier(b["g"], b["h"], b["gs"], b["hs"], b["u"], msm=oracle_msm)
        try:
            bv.add_wire_native([V], [blob], prepare="host")
            bv.verify()
        except Exception as e:
            assert "Proof invalid" in str(e)
            out.append(i)
    return out


def mixed_batch(batch, fmt="v1"):
    Vs, blobs = list(batch["Vs"]), list(batch[fmt])
    Vs[1] = batch["Vs"][2]                               # wrong commitment
    blobs[4] = t_hat_plus_one(blobs[4])
    blobs[5] = t_hat_plus_one(blobs[5])                  # two bad proofs in one group of four
    blobs[7] = flip_transcript_byte(blobs[7])
    blobs[10] = wrong_y(blobs[10]) if fmt == "v3" else off_curve_point(blobs[10])
    Vs[11] = batch["Vs"][0]                              # the last proof
    return Vs, blobs, [1, 4, 5, 7, 10, 11]


@pytest.mark.parametrize("group", [1, 4, None])
def test_locate_equals_the_proofs_rejected_one_by_one(batch, group):
    Vs, blobs, want = mixed_batch(batch)
    assert rejected_one_by_one(batch, Vs, blobs) == want
    bv = verifier(batch)
    try:
        assert bv.locate_wire(Vs, blobs, group=group) == want
        assert bv.locate_wire(batch["Vs"], batch["v1"], group=group) == []
        with pytest.raises(Exception, match="Proof invalid"):      # verify_wire is what it was
            bv.verify_wire(Vs, blobs)
        assert bv.verify_wire(batch["Vs"], batch["v1"]) is True
    finally:
        bv.release()


def test_default_group_is_the_largest_power_of_two_that_fits_one_launch(batch):
    bv = verifier(batch)
    assert bv.default_group() == 512                               # n = 8: 19 + 13 * 512 <= 8448 < 19 + 13 * 1024
    g64 = BatchRangeVerifier.__new__(BatchRangeVerifier)
    g64.n = 64
    assert g64.default_group() == 256 and g64.default_group(m=2) == 256
    bv.release()


@pytest.mark.parametrize("fmt", ["v1", "v2", "v3"])
def test_locate_in_every_wire_format(batch, fmt):
    Vs, blobs, want = mixed_batch(batch, fmt)
    bv = verifier(batch)
    try:
        assert bv.locate_wire(Vs, blobs, group=4) == want
        assert bv.locate_wire(batch["Vs"], batch[fmt], group=4) == []
    finally:
        bv.release()


def test_locate_aggregated_proofs(eng):
    """m = 2 values of 4 bits per proof; two commitments of one proof exchanged."""
    from oracle import bp_ref as R
    from oracle import cbind
    from helpers import gens
    from test_batch_verify_cpu import convert_proof, gpt
    m, bits = 2, 4
    rnd = random.Random(9)
    gs, hs = gens(m * bits, b"ags"), gens(m * bits, b"ahs")
    g, h, u = (R.elliptic_hash(s) for s in (b"ag", b"ah", b"au"))
    Vs_all, proofs = [], []
    for j in range(5):
        vs = [R.Zq(rnd.randrange(2 ** bits), Q) for _ in range(m)]
        gammas = [R.mod_hash(b"gl%d-%d" % (j, t), Q) for t in range(m)]
        Vs_all.append([gpt(R.commitment(g, h, v, ga)) for v, ga in zip(vs, gammas)])
        proofs.append(convert_proof(R.aggreg_range_prove(vs, bits, g, h, gs, hs, gammas, u, seed=b"ls%d" % j, multiexp=cbind.msm)))
    av = BatchRangeVerifier(gpt(g), gpt(h), [gpt(p) for p in gs], [gpt(p) for p in hs], gpt(u))
    try:
        for version in (1, 2, 3):
            blobs = [proof_to_bytes(pr, version=version) for pr in proofs]
            assert av.locate_wire(Vs_all, blobs, group=2) == []
            swapped = list(Vs_all)
            swapped[3] = [Vs_all[3][1], Vs_all[3][0]]
            assert av.locate_wire(swapped, blobs, group=2) == [3]
            assert av.locate_wire(swapped, blobs) == [3]
            packed = b"".join(V.to_le64() for Vg in swapped for V in Vg)
            assert av.locate_wire(packed, blobs, group=4) == [3]
    finally:
        av.release()


def test_row_chunks_do_not_change_the_group_values(eng, batch):
    """Option rp_rows = 5: 9 proofs are prepared in chunks of 5 + 4, the groups of four straddle them."""
    Vs, blobs = list(batch["Vs"][:9]), batch["v1"][:9]
    Vs[4] = batch["Vs"][0]
    ws = weights_for(9, 47)
    want = group_values(batch, Vs, blobs, ws, 4)
    assert want[0][1] != ZERO
    try:
        eng.set_option("rp_rows", 5)
        assert group_values(batch, Vs, blobs, ws, 4) == want
    finally:
        eng.set_option("rp_rows", 0)


@pytest.mark.parametrize("fmt", ["v1", "v2", "v3"])
def test_overlap_off_never_changes_a_result(eng, batch, fmt):
    """Option rp_overlap = 0 (tools and the benchmark library set it for measurements) moves the point decoding from the second lane
    to the ctx stream: behind the preparation kernels, and in group mode in FRONT of them, since k_rp_verdict reads the flags the
    decoding sets.  9 proofs of n = 8, once clean and once with an invalid point encoding in proof 6 (format 3: and a wrong y in proof
    2), through bpmi_rp_batch_prepare_dev and through the group values (groups of 4 over row chunks of 5 + 4, one wrong commitment):
    scalars, coefficients, points, verdicts, values and status bytes are the same bytes as with the default."""
    Vs, clean = list(batch["Vs"][:9]), list(batch[fmt][:9])
    Vs[4] = batch["Vs"][0]
    broken = list(clean)
    broken[6] = off_curve_point(clean[6])
    if fmt == "v3":
        broken[2] = wrong_y(clean[2])
    flagged = [2, 6] if fmt == "v3" else [6]
    ws, seed = weights_for(9, 61), b"\x47" * 32

    def run():
        return [(dev_prepare(eng, 8, 1, blobs, None, seed), group_values(batch, Vs, blobs, ws, 4)) for blobs in (clean, broken)]
    try:
        eng.set_option("rp_rows", 5)
        want = run()
        eng.set_option("rp_overlap", 0)
        got = run()
    finally:
        eng.set_option("rp_overlap", 1)
        eng.set_option("rp_rows", 0)
    for res in (want, got):
        (prep, (values, status)), (prep_b, (values_b, status_b)) = res
        assert prep[:2] == (0, -1) and status == bytes(9) and values[0] == ZERO and values[1] != ZERO
        assert prep_b[:2] == (0, flagged[0]) and [i for i in range(9) if status_b[i]] == flagged and all(status_b[i] & 2 for i in flagged)
        assert values_b == expected_values(batch, Vs, broken, ws, 4, skip=flagged)
    assert got == want


@pytest.mark.parametrize("group", [37, 38, 648, 649])
def test_either_side_of_the_switches_between_the_msm_routes(batch, group):
    """A group's MSM at n = 8 is 19 + 13 group pairs.  The light block shape holds 512 (group 37: 500 pairs, 38: 513 -- the shape of
    k_msm_mid), the one-launch kernel MID_NMAX = 8448 (648: 8443 pairs, 649: 8456 -- one msm_run per group).  650 proofs (six
    repeated) with one wrong commitment and fixed weights: every route gives partial_wire of the sub-batches."""
    count = 650
    blobs = [batch["v2"][i % 6] for i in range(count)]
    Vs = [batch["Vs"][i % 6] for i in range(count)]
    Vs[40] = batch["Vs"][5]
    Vs[649] = batch["Vs"][0]
    ws = weights_for(count, 53)
    values, status = group_values(batch, Vs, blobs, ws, group)
    assert status == bytes(count)
    assert values == expected_values(batch, Vs, blobs, ws, group)
    assert [t for t, v in enumerate(values) if v != ZERO] == sorted({40 // group, 649 // group})


def test_input_forms(eng, batch):
    """Packed commitments, a page-locked HostBuffer, and offsets into one buffer of proofs give what lists give."""
    Vs, blobs = list(batch["Vs"][:9]), batch["v2"][:9]
    Vs[7] = batch["Vs"][1]
    ws = weights_for(9, 59)
    want = group_values(batch, Vs, blobs, ws, 4)
    assert want[0][1] != ZERO
    packed = b"".join(V.to_le64() for V in Vs)
    joined, offs = b"".join(blobs), offsets_of(blobs)
    pinned_v = eng.host_alloc(len(packed))
    pinned_v.view[:] = packed
    pinned_b = eng.host_alloc(len(joined) + 100)
    pinned_b.view[:len(joined)] = joined
    try:
        assert group_values(batch, packed, blobs, ws, 4) == want
        assert group_values(batch, pinned_v, blobs, ws, 4) == want
        assert group_values(batch, Vs, joined, ws, 4, offsets=offs) == want
        assert group_values(batch, pinned_v, pinned_b, ws, 4, offsets=offs) == want
        bv = verifier(batch)
        try:
            for args in ((Vs, blobs, None), (packed, blobs, None), (pinned_v, blobs, None), (Vs, joined, offs), (pinned_v, pinned_b, offs)):
                assert bv.locate_wire(args[0], args[1], offsets=args[2], group=4) == [7]
            assert bv.locate_wire([], []) == [] and bv.group_values_wire([], []) == ([], b"")
        finally:
            bv.release()
    finally:
        pinned_v.free()
        pinned_b.free()


def raw_call(eng, b, Vs, blobs, group, values=True, status=True, seed=bytes(range(32))):
    """bpmi_rp_batch_group_values_dev through ctypes alone."""
    n, m, count = 8, 1, len(blobs)
    npairs = count * (m + 6 + 2 * K)
    joined, offs = b"".join(blobs), (ctypes.c_uint64 * (count + 1))(*offsets_of(blobs))
    gens = b"".join(p.to_le64() for p in [b["g"], b["h"], b["u"]] + b["gs"] + b["hs"])
    d_gens, d_pts, d_scs = eng.upload(gens), eng.alloc(64 * npairs), eng.alloc(32 * npairs)
    per = max(1, min(group, count))
    vals, st = ctypes.create_string_buffer(64 * ((count + per - 1) // per)), ctypes.create_string_buffer(count)
    try:
        rc = eng.lib.bpmi_rp_batch_group_values_dev(eng.ctx, n, m, count, joined, len(joined), ctypes.cast(offs, ctypes.c_void_p), None, seed,
                                                    b"".join(V.to_le64() for V in Vs), d_gens.ptr, d_pts.ptr, d_scs.ptr, group,
                                                    ctypes.cast(vals, ctypes.c_void_p) if values else None, ctypes.cast(st, ctypes.c_void_p) if status else None)
        return rc, vals.raw, st.raw
    finally:
        for d in (d_gens, d_pts, d_scs):
            d.free()


def test_c_abi_alone(eng, batch):
    Vs, blobs = list(batch["Vs"][:6]), list(batch["v1"][:6])
    rc, vals, st = raw_call(eng, batch, Vs, blobs, 2)
    assert rc == 0 and vals == bytes(64 * 3) and st == bytes(6)
    Vs[3] = batch["Vs"][0]
    blobs[4] = flip_transcript_byte(blobs[4])
    rc, vals, st = raw_call(eng, batch, Vs, blobs, 2)
    assert rc == 0 and st == bytes([0, 0, 0, 0, 1, 0])
    assert vals[:64] == ZERO and vals[64:128] != ZERO and vals[128:] == ZERO
    rc, vals, st = raw_call(eng, batch, Vs, blobs, 1)
    assert rc == 0 and [t for t in range(6) if vals[64 * t: 64 * t + 64] != ZERO] == [3] and st[4] == 1
    try:                                                  # a profiling run of one role never reads as valid
        eng.set_option("rp_only_role", 1)
        rc, vals, st = raw_call(eng, batch, batch["Vs"][:6], batch["v1"][:6], 2)
        assert rc == 0 and 0 not in st
    finally:
        eng.set_option("rp_only_role", -1)


def test_argument_errors_are_not_verdicts(eng, batch):
    Vs, v1, v2 = batch["Vs"][:6], batch["v1"][:6], batch["v2"][:6]
    assert raw_call(eng, batch, Vs, v1, 0)[0] == -3                              # BPMI_E_ARG
    assert raw_call(eng, batch, Vs, v1, 2, values=False)[0] == -3
    assert raw_call(eng, batch, Vs, v1, 2, status=False)[0] == -3
    assert raw_call(eng, batch, Vs, v2[:3] + [v1[3]] + v2[4:], 2)[0] == -3
    bv = verifier(batch)
    try:
        with pytest.raises(EngineError, match="group must be at least 1"):
            bv.group_values_wire(Vs, v1, group=0)
        with pytest.raises(EngineError, match="mixed wire formats: proof 3 is format 1 in a format-2 batch"):
            bv.group_values_wire(Vs, v2[:3] + [v1[3]] + v2[4:], group=2)
        with pytest.raises(EngineError, match="mixed wire formats: proof 2 is format 2 in a format-1 batch"):
            bv.locate_wire(Vs, v1[:2] + [v2[2]] + v1[3:])
        assert bv.locate_wire(Vs, v1) == []                                      # the ctx is usable after the errors
    finally:
        bv.release()
