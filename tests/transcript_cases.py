"""Inputs that put the device's transcript reader (csrc/rp_batch_kernels.hpp: the deferred SHA-256, the unaligned loads, the item
walker, the decimal reader, the format-2/3 expander; reused unchanged by csrc/ipa_packed_kernels.hpp) at every block phase, byte
alignment and edge value -- built in pure Python from ONE oracle proof per family, with every hash recomputed through hashlib
(oracle.bp_ref.mod_hash), and the model of the decimal rule both headers state.  tests/test_transcript_cases_cpu.py checks the
builders and the cover without a GPU; tests/test_gpu_transcript_phases.py runs the device against them."""
import re
import struct
from base64 import b64encode

import ipa_packed_ref as PR
from oracle import bp_ref as R

Q = PR.Q
TWO256 = 1 << 256

# ---- padding bytes: any byte but '&', a repeating NON-constant pattern whose period (61) shares no factor with 4, 8 or 64, so that a
# load from the wrong offset cannot give the right bytes
_PAT = bytes(c for c in range(0x21, 0x7F) if c != 0x26)[:61]


def pattern(n, phase=0):
    return bytes(_PAT[(i + 7 * phase) % 61] for i in range(n))


def _x_text(prefix):
    return str(R.mod_hash(prefix, Q).x).encode()


# ---- range proofs, wire format 1 (rangeproofs/codec.py) --------------------------------------------------------------------------------
def rp_body(k):
    return 6 + 32 * (5 + k) + 33 * (6 + 2 * k)


def rp_split(blob):
    """(k, head as a bytearray, start, [three transcripts]) of a format-1 proof."""
    assert blob[:5] == b"BPRP1"
    k = blob[5]
    body = rp_body(k)
    (start,) = struct.unpack(">H", blob[body: body + 2])
    o, ts = body + 2, []
    for _ in range(3):
        (ln,) = struct.unpack(">I", blob[o: o + 4])
        ts.append(bytes(blob[o + 4: o + 4 + ln]))
        o += 4 + ln
    assert o == len(blob)
    return k, bytearray(blob[:body]), start, ts


def rp_join(head, start, ts):
    return bytes(head) + struct.pack(">H", start) + b"".join(struct.pack(">I", len(t)) + t for t in ts)


def _rehash_rounds(head, items, start, k):
    """Every x_i item of a Protocol-2 transcript recomputed front to back (ipa_packed_ref._rehash_from), each also written big-endian
    into the scalar section at byte 166 + 32 i."""
    for r in range(k):
        j = start + 3 * r + 2
        x = R.mod_hash(b"&".join(items[:j]) + b"&", Q).x
        items[j] = str(x).encode()
        head[166 + 32 * r: 198 + 32 * r] = x.to_bytes(32, "big")


def rp_v1_variant(blob, pad0, pad1, pad2):
    """Item 0 of the three transcripts lengthened by pad0 / pad1 / pad2 pattern bytes.  The range-proof transcript's item 0 is neither
    checked nor hashed (it only shifts what lies behind it); the Protocol-1 challenge (item 1) and every x_i of Protocol 2 are
    recomputed, the x_i also in the scalar section; the three length fields follow."""
    k, head, start, ts = rp_split(blob)
    it0, it1, it2 = (t.split(b"&") for t in ts)
    it0[0] += pattern(pad0, 1)
    it1[0] += pattern(pad1, 2)
    it1[1] = _x_text(it1[0] + b"&")
    assert start == 3
    it2[0] += pattern(pad2, 3)
    _rehash_rounds(head, it2, start, k)
    return rp_join(head, start, [b"&".join(it) for it in (it0, it1, it2)])


def rp_v1_set_item(blob, j, text):
    """Item j (3 = y, 4 = z, 7 = x) of the range-proof transcript replaced by arbitrary bytes; those items are outside every chain."""
    k, head, start, ts = rp_split(blob)
    items = ts[0].split(b"&")
    items[j] = bytes(text)
    return rp_join(head, start, [b"&".join(items), ts[1], ts[2]])


def hash_points(blob):
    """Every digest the preparation takes of a format-1 proof: [{name, msg_len, ts_off, feed}] -- the message of mod_hash (the "1" in
    front of it not counted), the blob byte offset of the transcript it is taken over, and (fill & 3, off & 7) at the start of the
    incremental sha_feed that leads to it (fill: bytes in the SHA block, the "1" included; off: blob offset of the first byte fed)."""
    k, head, start, ts = rp_split(blob)
    off1 = len(head) + 2 + 4 + len(ts[0]) + 4
    off2 = off1 + len(ts[1]) + 4
    out = [dict(name="p1", msg_len=len(ts[1].split(b"&")[0]) + 1, ts_off=off1, feed=(1, off1 & 7))]
    out += _round_points(ts[2], start, k, off2)
    return out


def _round_points(tr, start, k, ts_off, tag="round"):
    items, out, hashed = tr.split(b"&"), [], 0
    for r in range(k):
        upto = len(b"&".join(items[: start + 3 * r + 2])) + 1
        out.append(dict(name="%s%d" % (tag, r), msg_len=upto, ts_off=ts_off, feed=((1 + hashed) & 3, (ts_off + hashed) & 7)))
        hashed = upto
    return out


# ---- range proofs, wire formats 2 and 3 -----------------------------------------------------------------------------------------------------
def rp_v2_variant(blob_v2, seed0, seed1, y=None, z=None, x=None, identity_L0=False):
    """A format-2 proof with the given seeds and free challenges (32-byte fields; None: as in blob_v2).  x_ip and every x_i are
    recomputed from the text codec.wire_v2_to_v1 writes for the new seed1 (with identity_L0: over 33 zero bytes for L_0), and written where
    they live: x_ip in the challenge section, the x_i in the scalar section."""
    from bulletproofs_amd.rangeproofs.codec import wire_v2_to_v1
    assert blob_v2[:5] == b"BPRP2"
    k = blob_v2[5]
    body = rp_body(k)
    b = bytearray(blob_v2[: body + 128])
    if identity_L0:
        at = 6 + 32 * (5 + k) + 33 * 6
        b[at: at + 33] = bytes(33)
    for j, v in enumerate((y, z, x)):
        if v is not None:
            b[body + 32 * j: body + 32 * j + 32] = int(v).to_bytes(32, "big")
    x_ip = R.mod_hash(b64encode(seed1) + b"&", Q).x
    b[body + 96: body + 128] = x_ip.to_bytes(32, "big")
    tail = struct.pack(">H", len(seed0)) + seed0 + struct.pack(">H", len(seed1)) + seed1
    keep = [b[body + 32 * j: body + 32 * j + 32] for j in range(3)]
    for j in range(3):                               # the text of the chain does not depend on y, z, x: expand with values the codec takes
        b[body + 32 * j: body + 32 * j + 32] = (1).to_bytes(32, "big")
    _, head, start, ts = rp_split(wire_v2_to_v1(bytes(b) + tail))
    items = ts[2].split(b"&")
    _rehash_rounds(b, items, start, k)
    for j in range(3):
        b[body + 32 * j: body + 32 * j + 32] = keep[j]
    return bytes(b) + tail


def rp_v3_of(blob_v2, ys):
    """The format-3 proof of a format-2 one: ys = the 32-byte big-endian y coordinates of its 6 + 2k points (zero is written for a
    point whose encoding is the identity's 33 zero bytes)."""
    k = blob_v2[5]
    at, out = 6 + 32 * (5 + k), []
    for j in range(6 + 2 * k):
        ident = blob_v2[at + 33 * j: at + 33 * j + 33] == bytes(33)
        out.append(bytes(32) if ident else bytes(ys[32 * j: 32 * j + 32]))
    return b"BPRP3" + bytes(blob_v2[5:]) + b"".join(out)


def v3_ys(blob_v3):
    k = blob_v3[5]
    return bytes(blob_v3[len(blob_v3) - 32 * (6 + 2 * k):])


# ---- packed inner-product proofs ----------------------------------------------------------------------------------------------------------
def _rewrite_xs(pk, i, start):
    k = pk.k
    pk.trs[i] = PR._rehash_from(pk.trs[i], start, k)
    items = pk.trs[i].split(b"&")
    pk.xs[32 * k * i: 32 * k * (i + 1)] = b"".join(PR.le32(int(items[start + 3 * r + 2])) for r in range(k))


def ipa_variant(pk, i, prefix):
    """Proof i of a Protocol-2 Packed as a one-proof Packed with the given transcript prefix (None or b"": none; otherwise items that
    end with '&'): start = the number of prefix items, the chain re-hashed and xs rewritten (as mut_l_replaced_rehashed does)."""
    assert pk.protocol == 2
    s = 1 if pk.starts is None else pk.starts[i]
    out = pk.subset([i])
    rounds = pk.trs[i].split(b"&")[s:]
    head = b"&" + (prefix or b"")
    assert head.endswith(b"&")
    out.trs[0] = head + b"&".join(rounds)
    out.starts = [len(head.split(b"&")) - 1]
    _rewrite_xs(out, 0, out.starts[0])
    return out


def ipa1_variant(pk, i, item0, item1):
    """Proof i of a Protocol-1 Packed with the given items 0 and 1: item 2 = str(mod_hash(item 1 + "&")), the rounds re-hashed."""
    assert pk.protocol == 1 and b"&" not in item0 + item1
    out = pk.subset([i])
    items = pk.trs[i].split(b"&")
    items[0], items[1] = item0, item1
    items[2] = _x_text(item1 + b"&")
    out.trs[0] = b"&".join(items)
    _rewrite_xs(out, 0, 3)
    return out


def ipa_join(pks):
    """One Packed from one-proof Packeds of the same k and protocol."""
    out = PR.Packed(pks[0].k, pks[0].protocol)
    for p in pks:
        assert p.count == 1 and (p.k, p.protocol) == (out.k, out.protocol)
        out.count += 1
        for name in ("ab", "xs", "lr", "P", "c", "head"):
            getattr(out, name).extend(getattr(p, name))
        if out.protocol == 2:
            out.u += p.u
        out.trs.append(p.trs[0])
    if out.protocol == 1:
        out.u = bytearray(pks[0].u)
    else:
        out.starts = [p.starts[0] for p in pks]
    return out


def ipa_hash_points(tr, start, k, protocol):
    """hash_points for one packed proof: the transposed transcript starts at offset 0 of its own rows, so ts_off is 0 for the rounds and
    the offset of item 1 inside the transcript for Protocol 1's challenge (which is hashed from there)."""
    out = []
    if protocol == 1:
        items = tr.split(b"&")
        b1 = len(items[0]) + 1
        out.append(dict(name="p1", msg_len=len(items[1]) + 1, ts_off=b1, feed=(1, b1 & 7)))
    return out + _round_points(tr, start, k, 0)


# ---- the sweeps (the same lists on the CPU and on the GPU) -------------------------------------------------------------------------------
RP_PAD0 = tuple(range(8))
# pad1 = pad2: two full turns of the 64-byte block, and the seven values that fill the cells the recomputed x_i's changing digit counts
# left empty (round 1: fill 47; round 2: fills 4, 12, 17, 23, 44, 53)
RP_PADS = tuple(range(128)) + (137, 145, 150, 156, 157, 180, 313)


def rp_phase_sweep(blob):
    return [rp_v1_variant(blob, pad0, p, p) for p in RP_PADS for pad0 in RP_PAD0]


IPA2_ONE_ITEM = tuple(range(128)) + (182,)          # 182: round 1 at fill 59, which two turns left empty
IPA2_TWO_ITEMS = tuple(range(16))
IPA1_ITEM0 = tuple(range(8))
IPA1_ITEM1 = tuple(range(64))


def ipa2_prefixes():
    return [b"", None] + [pattern(p, 4) + b"&" for p in IPA2_ONE_ITEM] + [pattern(p, 5) + b"&" + pattern(2 * p + 1, 6) + b"&" for p in IPA2_TWO_ITEMS]


def ipa2_phase_sweep(pk):
    return ipa_join([ipa_variant(pk, 0, pre) for pre in ipa2_prefixes()])


def ipa1_phase_sweep(pk):
    return ipa_join([ipa1_variant(pk, 0, pattern(a, 7), pattern(b, 8)) for a in IPA1_ITEM0 for b in IPA1_ITEM1])


# ---- the decimal rule of both headers: "canonical decimal -> value mod q; not canonical, or >= 2^256: refused" ----------------------------
_CANONICAL = re.compile(rb"0|[1-9][0-9]{0,77}")


def decimal_model(item):
    if not _CANONICAL.fullmatch(bytes(item)):
        return None
    v = int(bytes(item))
    return v % Q if v < TWO256 else None


# what a value that is 0 mod q means for each item the table is applied to (item index of the range-proof transcript -> verdict, reason)
ZERO_RULE = {
    3: (False, "y is inverted (y^-i scales the hs side): both headers refuse it -- 'a zero challenge cannot come out of mod_hash'"),
    4: (True, "z is only multiplied and added (delta, z^2, w2 z): neither header looks at its value, as the reference's verifier does not"),
    7: (True, "x is only multiplied (T1, T2, S scalars): neither header looks at its value, as the reference's verifier does not"),
}
ROLES = (3, 4, 7)                    # y, z, x


def decimal_accepts(item, j):
    v = decimal_model(item)
    return v is not None and (v != 0 or ZERO_RULE[j][0])


_NON_DIGITS = (b"/", b":", b" ", b"+", b"-", b"a", b"\x00", b"\x7f", b"\x80", b"\xff")


def _decimal_rows():
    rows = []
    for L in range(1, 79):
        rows.append(("1e%d" % (L - 1), b"1" + b"0" * (L - 1)))
        if L <= 77:
            rows.append(("9x%d" % L, b"9" * L))
    for name, v in (("10^77", 10 ** 77), ("2^256-1", TWO256 - 1), ("2^256", TWO256), ("2^256+1", TWO256 + 1), ("10^78-1", 10 ** 78 - 1), ("10^78", 10 ** 78),
                    ("q-1", Q - 1), ("q", Q), ("q+1", Q + 1), ("q+5", Q + 5), ("5", 5)):
        rows.append((name, str(v).encode()))
    rows += [("0", b"0"), ("00", b"00"), ("01", b"01"), ("empty", b"")]
    for digits in (b"12345678901234567890", b"1234567890123"):      # 8 + 8 + a right-aligned chunk of 4; 8 + a right-aligned chunk of 5
        for c in _NON_DIGITS:
            for pos in range(len(digits)):
                rows.append(("%d-digits-%02x-at-%d" % (len(digits), c[0], pos), digits[:pos] + c + digits[pos + 1:]))
    rows.append(("trailing-newline", b"12345\n"))
    return rows


DECIMAL_ROWS = _decimal_rows()
DECIMAL_ROW = dict(DECIMAL_ROWS)
# by the model: 163 rows have a value (two of them, "q" and "0", the value 0), 338 have none
DECIMAL_VALUED, DECIMAL_REFUSED = 163, 338


def decimal_cases(blob):
    """(accepted, refused): lists of (row name, item index, proof) over every row and y, z, x in turn."""
    acc, ref = [], []
    for name, item in DECIMAL_ROWS:
        for j in ROLES:
            (acc if decimal_accepts(item, j) else ref).append((name, j, rp_v1_set_item(blob, j, item)))
    return acc, ref


# ---- the expander table (formats 2 and 3) -----------------------------------------------------------------------------------------------------
V2_VALUES = [1, 9, 10, 10 ** 9 - 1, 10 ** 9, 10 ** 9 + 1, 10 ** 18, 10 ** 36 + 1, 5 * 10 ** 45 + 7 * 10 ** 9] + \
            [v for j in range(1, 78) for v in (10 ** j, 10 ** j - 1)] + [Q - 1]
V2_REFUSED_VALUES = [Q, Q + 1, TWO256 - 1]
V2_SEED_LENGTHS = tuple(range(24))


def _seed(n, phase):
    return bytes((37 * i + 11 * phase + 5) & 0xFF for i in range(n))


def v2_seed_sweep(blob_v2):
    """seed0 of 0..23 bytes with seed1 fixed, then seed1 of 0..23 bytes with seed0 fixed; two more proofs with the identity for L_0."""
    out = [rp_v2_variant(blob_v2, _seed(n, 1), b"fixed") for n in V2_SEED_LENGTHS]
    out += [rp_v2_variant(blob_v2, b"fixed-0", _seed(n, 2)) for n in V2_SEED_LENGTHS]
    out += [rp_v2_variant(blob_v2, _seed(5, 3), _seed(7, 4), identity_L0=True), rp_v2_variant(blob_v2, b"", b"", identity_L0=True)]
    return out


def v2_value_sweep(blob_v2, j):
    """Challenge j (0 = y, 1 = z, 2 = x) takes every value of V2_VALUES, each with seed lengths 0, 1, 2 mod 3 (the three base64 tails in
    front of the item, in either transcript)."""
    out = []
    for t, v in enumerate(V2_VALUES):
        for s in range(3):
            kw = {"yzx"[j]: v}
            out.append(rp_v2_variant(blob_v2, _seed(3 * (t % 5) + s, 5), _seed(3 * (t % 4) + (s + t) % 3, 6), **kw))
    return out


def v2_refused(blob_v2):
    """[(challenge index, value, proof)]: y, z or x not below q in the 32-byte field."""
    return [(j, v, rp_v2_variant(blob_v2, b"s0", b"s1", **{"yzx"[j]: v})) for j in range(3) for v in V2_REFUSED_VALUES]
