"""The case table of tests/point_edge_cases.py has what it promises, and the Python single-point decoders (ec.Point,
utils/pointcodec.bytes_to_point) accept exactly what strict decoding accepts: they used to take x + p, y + p and any tag byte,
which gave a Point that is != the canonical one and reaches the device with a coordinate >= p."""
import pytest

import bulletproofs_amd  # noqa: F401
from bulletproofs_amd.ec import Point, secp256k1
from bulletproofs_amd.utils.pointcodec import bytes_to_point, point_to_bytes

import point_edge_cases as E

P = E.P


def test_the_references_on_known_points():
    G = (secp256k1.gx, secp256k1.gy)
    assert P == secp256k1.p and E.EDGE == 2**256 - P
    assert E.decode_ref(E.enc(2, G[0])) == G[0].to_bytes(32, "little") + G[1].to_bytes(32, "little")      # G's y is even
    assert E.decode_ref(E.enc(3, G[0])) == G[0].to_bytes(32, "little") + (P - G[1]).to_bytes(32, "little")
    assert E.decode_ref(bytes(33)) == bytes(64) and E.decode_ref(b"\x00" + bytes(31) + b"\x01") is None
    assert E.decode_ref(E.enc(2, 0)) is None and E.decode_ref(E.enc(2, 5)) is None and E.decode_ref(E.enc(4, G[0])) is None
    assert [y for _, y in E.tiny_y_points()[::2]] == [1, 6, 11, 13, 17, 20]
    assert E.tiny_y_points()[0][0] == 0x1fe1e5ef3fceb5c135ab7741333ce5a6e80d68167653f6b2b24bcbcfaaaff507
    assert [x for x in range(23) if E.x_is_valid(x)] == [1, 2, 3, 4, 6, 8, 12, 13, 14, 16, 20, 22]
    assert [d for d in range(1, 23) if E.x_is_valid(P - d)][:8] == [3, 4, 10, 12, 13, 16, 19, 22]
    le = lambda x, y: x.to_bytes(32, "little") + y.to_bytes(32, "little")
    assert E.valid_ref(bytes(64)) and E.valid_ref(le(*G)) and E.valid_ref(le(G[0], P - G[1]))
    assert not E.valid_ref(le(G[0], G[1] + 1)) and not E.valid_ref(le(P, P)) and not E.valid_ref(le(0, P)) and not E.valid_ref(le(P, 0))
    assert not E.valid_ref(le(1 + P, int.from_bytes(E.decode_ref(E.enc(2, 1))[32:], "little")))
    y32 = G[1].to_bytes(32, "big")
    assert E.hint_ref(E.enc(2, G[0]), y32) and not E.hint_ref(E.enc(3, G[0]), y32) and not E.hint_ref(E.enc(2, G[0]), bytes(32))
    assert E.hint_ref(bytes(33), bytes(32)) and not E.hint_ref(bytes(33), y32)
    x1, _ = E.tiny_y_points()[0]
    assert E.hint_ref(E.enc(3, x1), (1).to_bytes(32, "big")) and not E.hint_ref(E.enc(2, x1), (1 + P).to_bytes(32, "big"))


def test_the_table_has_the_cases_it_promises():
    table = E.encodings()
    assert len(table) < 6000 and all(len(e) == 33 for _, e in table)
    dec = [E.decode_ref(e) for _, e in table]
    body = [(e, d) for (_, e), d in zip(table, dec) if e[0] != 0]
    assert sum(d is not None for _, d in body) >= 100 and sum(d is None for _, d in body) >= 100
    bits = [E.decode_ref(E.enc(2, 1 << b)) for b in range(256)]
    assert sum(d is not None for d in bits) == 130
    aliases = [e for _, e in table if E.is_alias(e)]
    assert len(aliases) >= 10 and all(E.decode_ref(e) is None for e in aliases)
    assert sum(d is not None and E.has_tiny_y(d) for d in dec) >= 12
    for (label, e), d in zip(table, dec):
        if d is not None and d != bytes(64):
            x, y = int.from_bytes(d[:32], "little"), int.from_bytes(d[32:], "little")
            assert x < P and y < P and E.on_curve(x, y) and (y & 1) == (e[0] & 1) and x == int.from_bytes(e[1:], "big"), label
    # the wrong tag of a tiny-y point decodes to the other root
    for x, y in E.tiny_y_points():
        assert int.from_bytes(E.decode_ref(E.enc(3 - (y & 1), x))[32:], "little") == P - y
    pts = E.points64()
    assert sum(E.valid_ref(b) for _, b in pts) >= 100 and sum(not E.valid_ref(b) for _, b in pts) >= 100
    # aliases in both coordinates, which only the range check can reject
    unreduced = [b for _, b in pts if not E.valid_ref(b) and E.on_curve(int.from_bytes(b[:32], "little"), int.from_bytes(b[32:], "little"))]
    assert sum(int.from_bytes(b[:32], "little") >= P for b in unreduced) >= 100 and sum(int.from_bytes(b[32:], "little") >= P for b in unreduced) >= 12


def test_bytes_to_point_is_strict_and_round_trips():
    for label, e in E.encodings():
        want = E.decode_ref(e)
        if want is None:
            with pytest.raises(ValueError):
                bytes_to_point(e)
            continue
        pt = bytes_to_point(e)
        assert pt.to_le64() == want, label
        if want == bytes(64):
            assert pt == Point.IDENTITY_ELEMENT and bytes_to_point(point_to_bytes(pt)) == pt
        else:
            assert point_to_bytes(pt) == e, label
    for bad in (b"", b"\x02", b"\x00\x00", b"\x02" + bytes(30) + b"\x01", b"\x02" + bytes(32) + b"\x01", bytes(34)):
        with pytest.raises(ValueError):
            bytes_to_point(bad)


def test_point_rejects_coordinates_outside_the_field():
    for label, b in E.points64():
        x, y = int.from_bytes(b[:32], "little"), int.from_bytes(b[32:], "little")
        if E.valid_ref(b):
            pt = Point(x, y, secp256k1)
            assert pt.to_le64() == b and pt == Point.from_le64(b), label
        else:
            with pytest.raises(ValueError, match="not on curve"):
                Point(x, y, secp256k1)
    x, y = E.tiny_y_points()[0]
    for bad in ((x + P, y), (x, y + P), (x - P, y), (x, y - P), (x, -y), (P, P)):
        with pytest.raises(ValueError, match="not on curve"):
            Point(*bad, secp256k1)
    with pytest.raises(ValueError):
        Point(0, 0, secp256k1)
    assert Point(0, 0, None) == Point.IDENTITY_ELEMENT


@pytest.mark.parametrize("fmt", [1, 2, 3])
def test_host_preparation_judges_substituted_points_like_the_reference(fmt):
    """The host twin of the device preparation (bpmi_rp_batch_prepare) over a 4-proof batch with one point slot overwritten -- every
    alias and tiny-y case of the table.  Format 3: it names the proof exactly when hint_ref rejects (rp_wire_v2_host.hpp hint_ok:
    its own "< p" and parity checks).  Formats 1 / 2: it leaves encodings to the decompression and the slots are in no transcript,
    so every batch passes -- which is what makes the device's verdict in tests/test_gpu_point_decoders.py the decoder's alone."""
    import random
    from bulletproofs_amd.rangeproofs.codec import proof_to_bytes
    from helpers import Q
    from test_gpu_batch_dev import _v2, _v3, host_prepare, make_batch
    b = make_batch(4, n=8)
    blobs = {1: [proof_to_bytes(pr) for pr in b["proofs"]], 2: _v2(b["proofs"]), 3: _v3(b["proofs"])}[fmt]
    rnd = random.Random(14)
    w = b"".join(rnd.randrange(1, Q).to_bytes(32, "little") for _ in range(16))
    t = E.encodings()
    cases = E.format_3_cases(t, True) if fmt == 3 else [c + (None,) for c in E.format_12_cases(t, True)]
    rejected = 0
    for i, (label, e, hint) in enumerate(cases):
        j, slot = i % 4, E.FREE_SLOTS[(i // 4) % 2]
        mutated = list(blobs)
        mutated[j] = E.substitute(mutated[j], slot, e, hint)
        rc, bad = host_prepare(8, 1, mutated, w, None)[:2]
        want = j if fmt == 3 and not E.hint_ref(e, hint) else -1
        assert rc == 0 and bad == want, "%s in proof %d: host names %d" % (label, j, bad)
        rejected += want >= 0
    assert rejected >= (300 if fmt == 3 else 0)
