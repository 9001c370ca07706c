"""Every decoder of untrusted point bytes, at the field boundary (tests/point_edge_cases.py): k_ec_decompress, the two branches of
k_ec_decompress_wire (square root for wire formats 1 / 2, checked y for format 3), and wire_point_valid on the host and in
k_ec_validate.  All of them check the curve equation modulo p, so only their carry chain "coordinate + 2^32 + 977 does not carry
out of 256 bits" rejects the second encoding (x0 + p, y) or (x, y0 + p) of a valid point -- and only the parity of the CANONICAL y
may choose the root.  The reference is the strict decoding of point_edge_cases (decode_ref / valid_ref / hint_ref), not the oracle,
which accepts unreduced coordinates like the implementation it mirrors; the oracle is the reference for group arithmetic only."""
import ctypes
import random

import pytest

import point_edge_cases as E
from helpers import Q
from oracle import cbind

pytestmark = pytest.mark.gpu

P = E.P
GUARD = 192
NPTS, FREE_SLOTS = E.NPTS, E.FREE_SLOTS


@pytest.fixture(scope="module")
def gp():
    import gpu_common
    return gpu_common


@pytest.fixture(scope="module")
def eng(gp):
    return gp.engine()


@pytest.fixture(scope="module")
def table():
    t = E.encodings()
    return t, [E.decode_ref(e) for _, e in t]


def _decompress_guarded(eng, comp, n):
    """bpmi_ec_decompress_batch into buffers with GUARD bytes of 0xA5 behind both outputs: nothing behind the last output may change."""
    out = ctypes.create_string_buffer(b"\xA5" * (64 * n + GUARD), 64 * n + GUARD)
    ok = ctypes.create_string_buffer(b"\xA5" * (n + GUARD), n + GUARD)
    assert eng.lib.bpmi_ec_decompress_batch(eng.ctx, comp, n, out, ok) == 0
    assert out.raw[64 * n:] == b"\xA5" * GUARD and ok.raw[n:] == b"\xA5" * GUARD, "bytes behind the outputs of %d points were written" % n
    return out.raw[:64 * n], ok.raw[:n]


def _assert_decoded(labels, want, out, ok):
    for i, (label, w) in enumerate(zip(labels, want)):
        assert ok[i] == (w is not None), "%s: ok = %d" % (label, ok[i])
        assert out[64 * i: 64 * i + 64] == (w if w is not None else bytes(64)), label


# ---- 1. k_ec_decompress -------------------------------------------------------------------------------------------------------------
def test_decompress_batch_decodes_the_whole_table(eng, table):
    t, want = table
    out, ok = _decompress_guarded(eng, b"".join(e for _, e in t), len(t))
    _assert_decoded([label for label, _ in t], want, out, ok)
    assert (out, ok) == eng.ec_decompress_batch_bytes(b"".join(e for _, e in t), len(t))


def test_decompress_batch_prefixes_end_on_an_alias_between_valid_points(eng, table):
    """Prefixes of a shuffled table that end inside, at and just behind a wave and a block; each ends on an alias x0 + p (invalid by
    the range check alone) whose neighbours in the wave are valid points.  The bytes behind the last output are guarded."""
    t, want = table
    idx = list(range(len(t)))
    random.Random(1).shuffle(idx)
    aliases = [i for i in idx if E.is_alias(t[i][1])]
    valid = [i for i in idx if want[i] is not None and want[i] != bytes(64)]
    for r, n in enumerate((1, 63, 64, 65, 255, 256, 257)):
        pick = idx[:n]
        pick[n - 1] = aliases[r]
        for back in (2, 3):
            if n - back >= 0:
                pick[n - back] = valid[2 * r + back]
        assert want[pick[-1]] is None and all(want[i] is not None for i in pick[-3:-1])
        out, ok = _decompress_guarded(eng, b"".join(t[i][1] for i in pick), n)
        _assert_decoded(["prefix %d: %s" % (n, t[i][0]) for i in pick], [want[i] for i in pick], out, ok)


# ---- 2. k_ec_decompress_wire --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wire():
    from bulletproofs_amd.rangeproofs.codec import proof_to_bytes
    from test_gpu_batch_dev import _v2, _v3, make_batch
    b = make_batch(4, n=8)
    rnd = random.Random(14)
    w = b"".join(rnd.randrange(1, Q).to_bytes(32, "little") for _ in range(16))
    return b, {1: [proof_to_bytes(pr) for pr in b["proofs"]], 2: _v2(b["proofs"]), 3: _v3(b["proofs"])}, w


@pytest.mark.parametrize("fmt", [1, 2, 3])
def test_wire_decoders_one_substituted_point_per_call(eng, wire, fmt):
    """One point slot of one proof of a 4-proof batch overwritten with a table encoding (format 3: and its hint), about 40 per
    format with every tiny-y case.  The slots are u_new / P_new, which no transcript holds: the byte-level checks do not see the
    substitution (asserted: the host twin of formats 1 / 2, which leaves encodings to the decompression, passes every batch), so the
    decoder alone decides.  Rejected by decode_ref / hint_ref: the device names that proof (format 3: so does the host twin, hint_ok);
    accepted -- a genuine but different point, whose proof fails in the MSM -- the device's verdict is the host twin's.
    include/bpmi.h leaves the decoded points of a rejected batch undefined ("no usable result"), so only verdicts are asserted; the
    decoded bytes are pinned by the accepted cases here and by the table test above.  About 80 prepare calls per format."""
    from test_gpu_batch_dev import dev_prepare, host_prepare
    _, blobs, w = wire
    t = E.encodings()
    cases = E.format_3_cases(t, False) if fmt == 3 else [c + (None,) for c in E.format_12_cases(t, False)]
    assert 40 <= len(cases) <= 75
    rejected = 0
    for i, (label, e, hint) in enumerate(cases):
        j, slot = i % 4, FREE_SLOTS[(i // 4) % 2]
        want_ok = E.hint_ref(e, hint) if fmt == 3 else E.decode_ref(e) is not None
        mutated = list(blobs[fmt])
        mutated[j] = E.substitute(mutated[j], slot, e, hint)
        h = host_prepare(8, 1, mutated, w, None)
        d = dev_prepare(eng, 8, 1, mutated, w, None)
        assert h[0] == 0 and d[0] == 0, label
        if fmt != 3:
            assert h[1] == -1, label
        if want_ok:
            assert d[1] == h[1] == -1, "%s in proof %d: device %d, host %d" % (label, j, d[1], h[1])
            want = E.decode_ref(e)
            at = 64 * (NPTS * j + slot)
            assert d[5][at: at + 64] == want, label
        else:
            rejected += 1
            assert d[1] == j, "%s in proof %d: device names %d" % (label, j, d[1])
            if fmt == 3:
                assert h[1] == j, "%s in proof %d: host names %d" % (label, j, h[1])
    assert rejected >= 10 and len(cases) - rejected >= 20


@pytest.mark.parametrize("fmt", [1, 2, 3])
def test_wire_decoders_every_alias_and_tiny_y_case_in_one_batch(eng, wire, fmt):
    """EVERY alias and tiny-y case of the table, one proof each, in one call that answers per proof (bpmi_rp_batch_group_values_dev,
    groups of one: status bit 1 = an invalid point encoding, set by k_ec_decompress_wire; bit 0 = a byte-level check, which a
    substitution in these slots never fails)."""
    from bulletproofs_amd.rangeproofs.batch import BatchRangeVerifier
    b, blobs, _ = wire
    t = E.encodings()
    cases = E.format_3_cases(t, True) if fmt == 3 else [c + (None,) for c in E.format_12_cases(t, True)]
    batch, want = [], []
    for i, (label, e, hint) in enumerate(cases):
        batch.append(E.substitute(blobs[fmt][i % 4], FREE_SLOTS[(i // 4) % 2], e, hint))
        want.append(E.hint_ref(e, hint) if fmt == 3 else E.decode_ref(e) is not None)
    bv = BatchRangeVerifier(b["g"], b["h"], b["gs"], b["hs"], b["u"])
    _, status = bv.group_values_wire([b["Vs"][i % 4] for i in range(len(batch))], batch, group=1)
    assert len(status) == len(cases)
    for (label, _, _), ok, st in zip(cases, want, status):
        assert (st & 2) == (0 if ok else 2) and (ok or st & 1 == 0) and (st == 0 or not ok), "%s: status %d" % (label, st)
    assert want.count(False) >= 100 and want.count(True) >= 24


# ---- 3. wire_point_valid: the host loop and k_ec_validate ---------------------------------------------------------------------------
HOST_MAX = 64                                    # csrc/point_check_host.hpp VALIDATE_HOST_MAX: bpmi_ec_sum checks up to 64 points on the host


@pytest.fixture(scope="module")
def good(gp):
    pts, _ = gp.rand_points(2 * HOST_MAX + 1, 23)
    rnd = random.Random(24)
    return cbind.pack_points(pts), cbind.pack_scalars([rnd.randrange(Q) for _ in pts])


def _put(blob, pos, xy64):
    return blob[: 64 * pos] + xy64 + blob[64 * pos + 64:]


def _split():
    pts = E.points64()
    return [c for c in pts if E.valid_ref(c[1])], [c for c in pts if not E.valid_ref(c[1])]


def test_ec_sum_host_side_check_refuses_exactly_the_invalid_points(eng, good):
    """bpmi_ec_sum of 64 points: wire_point_valid compiled for the host.  One bad point per call, first, last and in the middle."""
    lib, ctx = eng.lib, eng.ctx
    n = HOST_MAX
    base = good[0][: 64 * n]
    valid, bad = _split()
    for i, (label, xy) in enumerate(bad):
        pos = (0, n - 1, n // 2 - 1)[i % 3]
        out = ctypes.create_string_buffer(b"\x55" * 64, 64)
        assert lib.bpmi_ec_sum(ctx, _put(base, pos, xy), n, out) == -3, label
        assert b"pts[%d] is not a point of the curve" % pos in lib.bpmi_last_error(ctx), label
        assert out.raw == bytes(64), label
    ones = cbind.pack_scalars([1] * n)
    for at in range(0, len(valid), n - 2):
        chunk = valid[at: at + n - 2]
        blob = base[:64] + b"".join(xy for _, xy in chunk) + base[64 * (len(chunk) + 1):]
        out = ctypes.create_string_buffer(b"\x55" * 64, 64)
        assert lib.bpmi_ec_sum(ctx, blob, n, out) == 0, chunk[0][0]
        assert out.raw == cbind.msm_bytes(blob, ones, n, 8), chunk[0][0]


def test_validate_kernel_refuses_exactly_the_invalid_points(eng, good):
    """bpmi_msm of 129 points and bpmi_ec_sum of 65: k_ec_validate.  One bad point per call: first, last, and on both sides of the
    seam between the first two waves."""
    lib, ctx = eng.lib, eng.ctx
    n = 2 * HOST_MAX + 1
    pb, sb = good
    valid, bad = _split()
    for i, (label, xy) in enumerate(bad):
        pos = (0, n - 1, 63, 64)[i % 4]
        out = ctypes.create_string_buffer(b"\x55" * 64, 64)
        assert lib.bpmi_msm(ctx, _put(pb, pos, xy), sb, n, out) == -3, label
        assert b"pts[%d] is not a point of the curve" % pos in lib.bpmi_last_error(ctx), label
        assert out.raw == bytes(64), label
        if i % 8 == 0:                           # the same kernel behind bpmi_ec_sum, one point past the host loop's limit
            pos = (HOST_MAX, 0, 63)[(i // 8) % 3]
            out = ctypes.create_string_buffer(b"\x55" * 64, 64)
            assert lib.bpmi_ec_sum(ctx, _put(pb[: 64 * (HOST_MAX + 1)], pos, xy), HOST_MAX + 1, out) == -3, label
            assert b"pts[%d] is not a point of the curve" % pos in lib.bpmi_last_error(ctx), label
            assert out.raw == bytes(64), label
    m = len(valid)
    assert m > HOST_MAX
    blob = b"".join(xy for _, xy in valid)
    rnd = random.Random(25)
    sc = cbind.pack_scalars([rnd.randrange(Q) for _ in range(m)])
    out = ctypes.create_string_buffer(b"\x55" * 64, 64)
    assert lib.bpmi_msm(ctx, blob, sc, m, out) == 0 and out.raw == cbind.msm_bytes(blob, sc, m, 8)
    half = blob[: 64 * (HOST_MAX + 1)]
    assert lib.bpmi_ec_sum(ctx, half, HOST_MAX + 1, out) == 0 and out.raw == cbind.msm_bytes(half, cbind.pack_scalars([1] * (HOST_MAX + 1)), HOST_MAX + 1, 8)


# ---- 4. the edge points as operands -------------------------------------------------------------------------------------------------
def test_edge_points_as_operands_of_the_group_kernels(eng):
    """The valid points with x <= 256, x >= p - 256 or a tiny y, and their negatives -- limbs mostly zero or mostly ones --
    through the scalar-multiplication ladder, the block sum and MSMs of 64 and 5000 pairs, against the C oracle."""
    ops = E.operand_points()
    n = len(ops)
    assert n >= 400
    pb = b"".join(xy for _, xy in ops)
    rnd = random.Random(26)
    ks = [rnd.randrange(Q) for _ in range(n)]
    ks[:6] = [0, 1, 2, Q - 1, Q - 2, 3]
    sb = cbind.pack_scalars(ks)
    want = ctypes.create_string_buffer(64 * n)
    cbind.lib().orc_ec_mul_batch(pb, sb, n, 8, want)
    got = eng.ec_mul_batch_bytes(pb, sb, n)
    for i, (label, _) in enumerate(ops):
        assert got[64 * i: 64 * i + 64] == want.raw[64 * i: 64 * i + 64], "%s times 0x%x" % (label, ks[i])
    ones = cbind.pack_scalars([1] * n)
    assert eng.ec_sum_bytes(pb, n) == bytes(64)                              # every point is followed by its negative
    for part in (pb[: 64 * 200], b"".join(xy for _, xy in ops[::2]), b"".join(xy for _, xy in ops[1::2]), pb[64 * 3: 64 * 40]):
        m = len(part) // 64
        assert eng.ec_sum_bytes(part, m) == cbind.msm_bytes(part, ones, m, 8)
    assert eng.msm_bytes(pb[: 64 * 64], sb[: 32 * 64], 64) == cbind.msm_bytes(pb[: 64 * 64], sb[: 32 * 64], 64, 8)
    big = 5000
    pbig = (pb * (big // n + 1))[: 64 * big]
    sbig = cbind.pack_scalars([rnd.randrange(Q) for _ in range(big)])
    assert eng.msm_bytes(pbig, sbig, big) == cbind.msm_bytes(pbig, sbig, big, 8)
