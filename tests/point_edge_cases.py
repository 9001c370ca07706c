"""Point encodings at the field boundary, for every decoder of untrusted bytes (tests/test_point_edge_cases_cpu.py,
tests/test_gpu_point_decoders.py).  Pure Python integers; imports neither the product nor the oracle.

The decoders check the curve equation modulo p, so the range check "coordinate < p" is the ONLY thing that tells the second
encoding (x0 + p, y) or (x, y0 + p) of a valid point from the point itself -- and x0 + p fits 256 bits only for
x0 < 2^32 + 977.  Likewise the parity of a y within 2^32 + 977 of 0 or of p is the parity of the canonical y, not of any other
representative.  Random points never land at either edge; these are constructed: p = 7 (mod 9), so a cubic residue a has the
cube root a^((p+2)/9), which gives the x of a point with a chosen tiny y.

The references here state strict SEC1 decoding as the library documents it (include/bpmi.h, csrc/point_kernels.hpp); the oracle
under oracle/ mirrors the reference implementation, which accepts unreduced coordinates, and is NOT the reference for these cases."""
import functools
import random

P = 2**256 - 2**32 - 977
EDGE = 2**32 + 977            # 2^256 - p: v + p fits 256 bits exactly when v < EDGE
TWO256 = 1 << 256


def _sqrt(a):
    a %= P
    y = pow(a, (P + 1) // 4, P)
    return y if y * y % P == a else None


def _cbrt(a):
    a %= P
    r = pow(a, (P + 2) // 9, P)
    return r if pow(r, 3, P) == a else None


def on_curve(x, y):
    return (y * y - x * x * x - 7) % P == 0


def _le(x, y):
    return x.to_bytes(32, "little") + y.to_bytes(32, "little")


def enc(tag, x):
    return bytes([tag]) + x.to_bytes(32, "big")


def decode_ref(enc33):
    """Strict SEC1: 64 bytes (x | y, 32 bytes little-endian each; the identity is 64 zero bytes) or None."""
    assert len(enc33) == 33
    tag, x = enc33[0], int.from_bytes(enc33[1:], "big")
    if tag == 0:
        return bytes(64) if x == 0 else None
    if tag not in (2, 3) or x >= P:
        return None
    y = _sqrt(x * x * x + 7)
    if y is None:
        return None
    if (y & 1) != (tag & 1):
        y = P - y
    return _le(x, y)


def valid_ref(xy64):
    """The 64-byte form: the identity, or both coordinates below p and on the curve."""
    assert len(xy64) == 64
    x, y = int.from_bytes(xy64[:32], "little"), int.from_bytes(xy64[32:], "little")
    if x == 0 and y == 0:
        return True
    return x < P and y < P and on_curve(x, y)


def hint_ref(enc33, y32):
    """Wire format 3: is y32 (big-endian) THE y coordinate of the encoding?"""
    assert len(enc33) == 33 and len(y32) == 32
    tag, x, y = enc33[0], int.from_bytes(enc33[1:], "big"), int.from_bytes(y32, "big")
    if tag == 0:
        return x == 0 and y == 0
    return tag in (2, 3) and x < P and y < P and (y & 1) == (tag & 1) and on_curve(x, y)


def x_is_valid(x):
    return x < P and _sqrt(x * x * x + 7) is not None


@functools.lru_cache(maxsize=None)
def tiny_y_points():
    """(x, y) for the first six y >= 1 whose y^2 - 7 has a cube root, each with y and with p - y: 12 points whose canonical y is
    within 2^32 + 977 of 0 or of p."""
    out, y = [], 1
    while len(out) < 12:
        x = _cbrt(y * y - 7)
        if x is not None:
            assert on_curve(x, y)
            out += [(x, y), (x, P - y)]
        y += 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def small_points():
    """The valid points with a small coordinate: (x0, y0) for every x-coordinate x0 <= 256 (y0 the even root) and the tiny-y points."""
    out = []
    for x in range(257):
        y = _sqrt(x * x * x + 7)
        if y is not None:
            out.append(("x=%d" % x, x, y if y % 2 == 0 else P - y))
    for x, y in tiny_y_points():
        out.append(("tiny y=%s" % (y if y < EDGE else "p-%d" % (P - y)), x, y))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def near_p_points():
    """(label, x, y) for the x-coordinates p - d, d <= 256: limbs mostly ones."""
    out = []
    for d in range(1, 257):
        y = _sqrt((P - d) ** 3 + 7)
        if y is not None:
            out.append(("x=p-%d" % d, P - d, y))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def encodings():
    """The case table: a tuple of (label, 33 bytes).  Under 6000 entries."""
    t = []
    # small and large x, both tags
    for x in range(257):
        t += [("x=%d tag %d" % (x, tag), enc(tag, x)) for tag in (2, 3)]
    for d in range(1, 257):
        t += [("x=p-%d tag %d" % (d, tag), enc(tag, P - d)) for tag in (2, 3)]
    # tiny y: the tag of the canonical y, and the other tag (valid: it decodes to the other root)
    for x, y in tiny_y_points():
        name = str(y) if y < EDGE else "p-%d" % (P - y)
        t.append(("tiny y=%s right tag" % name, enc(2 + (y & 1), x)))
        t.append(("tiny y=%s wrong tag" % name, enc(3 - (y & 1), x)))
    # bit patterns
    for b in range(256):
        t += [("x=1<<%d tag %d" % (b, tag), enc(tag, 1 << b)) for tag in (2, 3)]
    for b in range(257):
        t += [("x=(1<<%d)-1 tag %d" % (b, tag), enc(tag, (1 << b) - 1)) for tag in (2, 3)]
    for i in range(8):
        t += [("x=0xFFFFFFFF<<%d tag %d" % (32 * i, tag), enc(tag, 0xFFFFFFFF << (32 * i))) for tag in (2, 3)]
    # aliases x0 + p of every valid x0 so far that has one in 256 bits, and the values around p and 2^256
    x0s = sorted({int.from_bytes(e[1:], "big") for _, e in t if e[0] in (2, 3)})
    for x0 in x0s:
        if x0 < EDGE and x_is_valid(x0):
            t += [("alias x=%d+p tag %d" % (x0, tag), enc(tag, x0 + P)) for tag in (2, 3)]
    for name, x in (("p", P), ("p+1", P + 1), ("2^256-1", TWO256 - 1), ("2^255", 1 << 255), ("2^256-978", TWO256 - 978),
                    ("2^256-977", TWO256 - 977), ("2^256-2^32", TWO256 - 2**32), ("p-1+2^32", P - 1 + 2**32)):
        t += [("x=%s tag %d" % (name, tag), enc(tag, x)) for tag in (2, 3)]
    # every tag byte over one valid x
    t += [("tag %d over x=1" % tag, enc(tag, 1)) for tag in range(256)]
    # identity variants
    t.append(("identity", bytes(33)))
    for pos in range(32):
        body = bytearray(32)
        body[pos] = 0x80 if pos % 2 else 0x01
        t.append(("tag 0 with body byte %d set" % pos, b"\x00" + bytes(body)))
    t += [("tag %d with a zero body" % tag, enc(tag, 0)) for tag in (2, 3)]
    # random
    rnd = random.Random(20261019)
    n = 0
    while n < 300:
        x = rnd.randrange(P)
        if x_is_valid(x):
            t.append(("random valid #%d" % n, enc(rnd.choice((2, 3)), x)))
            n += 1
    for i in range(300):
        t.append(("random x #%d" % i, enc(rnd.choice((2, 3, 2, 3, 2, 3, 0, 1, 4, 0x82)), rnd.randrange(TWO256))))
    assert len(t) < 6000
    return tuple(t)


def is_alias(e):
    """An encoding with tag 2 / 3 whose x is >= p and congruent to the x-coordinate of a point."""
    x = int.from_bytes(e[1:], "big")
    return e[0] in (2, 3) and x >= P and x_is_valid(x - P)


def has_tiny_y(xy64):
    y = int.from_bytes(xy64[32:], "little")
    return 0 < y < EDGE or 0 < P - y < EDGE


@functools.lru_cache(maxsize=None)
def points64():
    """(label, 64 bytes) around every valid small-coordinate point: the point and its negative (valid), its aliases (x0 + p, y0) and
    (x0, y0 + p) where they fit 256 bits, its neighbours (x0, y0 +- 1), and the aliases of the identity, which are not the identity."""
    t = []
    for name, x, y in small_points():
        t.append((name, _le(x, y)))
        t.append((name + " negated", _le(x, P - y)))
        if x + P < TWO256:
            t.append((name + " x+p", _le(x + P, y)))
            t.append((name + " x+p negated", _le(x + P, P - y)))
        for yy, what in ((y, "y"), (P - y, "(p-y)")):
            if yy + P < TWO256:
                t.append((name + " %s+p" % what, _le(x, yy + P)))
        t.append((name + " y+1", _le(x, y + 1)))
        t.append((name + " y-1", _le(x, y - 1)))
    t += [("(p, p)", _le(P, P)), ("(p, 0)", _le(P, 0)), ("(0, p)", _le(0, P)), ("(2^256-1, 2^256-1)", _le(TWO256 - 1, TWO256 - 1))]
    return tuple(t)


def operand_points():
    """(label, 64 bytes): the valid points with mostly-zero or mostly-one limbs (both roots), as operands of the group kernels."""
    out = []
    for name, x, y in small_points() + near_p_points():
        out += [(name, _le(x, y)), (name + " negated", _le(x, P - y))]
    return out


# ---- substitutions into the wire proofs of make_batch(4, n=8) (tests/test_batch_verify_cpu.py): 3 IPA rounds, 6 + 2k = 12 points ----
K, NPTS = 3, 12
PTS_AT = 6 + 32 * (5 + K)                        # every wire format holds the encodings here; format 3 ends with NPTS x 32 B of y
FREE_SLOTS = (4, 5)                              # u_new, P_new: in no transcript, so no byte-level check sees a substitution there


def substitute(blob, slot, e, hint=None):
    b = bytearray(blob)
    b[PTS_AT + 33 * slot: PTS_AT + 33 * slot + 33] = e
    if hint is not None:
        at = len(b) - 32 * NPTS + 32 * slot
        b[at: at + 32] = hint
    return bytes(b)


def _be_y(xy64):
    return xy64[32:][::-1]


def alias_encodings(t):
    return [(label, e) for label, e in t if is_alias(e)]


def tiny_encodings(t):
    return [(label, e) for label, e in t if label.startswith("tiny y=")]


def format_12_cases(t, every):
    """(label, encoding): every tiny-y encoding, the values around p and 2^256, tags and identity forms; every alias when `every`,
    else the aliases of the smallest and the largest x0 that have one."""
    aliases = alias_encodings(t)
    aliases.sort(key=lambda c: int.from_bytes(c[1][1:], "big"))
    chosen = aliases if every else aliases[:4] + aliases[-4:]
    extra = [c for c in t if c[0] in ("x=p tag 2", "x=p+1 tag 3", "x=2^256-1 tag 2", "x=2^256-977 tag 3", "x=0 tag 2", "x=5 tag 3", "tag 4 over x=1",
                                      "tag 130 over x=1", "identity", "tag 0 with body byte 31 set", "x=p-3 tag 2", "x=p-1 tag 3")]
    assert len(extra) == 12 and len(tiny_encodings(t)) == 24 and len(aliases) >= 10
    return tiny_encodings(t) + chosen + extra


def format_3_cases(t, every):
    """(label, encoding, hint): as above with the y that decode_ref gives (for an alias: the y of x0 with the tag's parity, so that
    only x >= p is wrong), and for the tiny-y points the hints that only one check can reject: y0 + p under the tag of ITS parity
    (range), the right y under the other tag (parity), zero, p, p + 1, 2^256 - 1."""
    cases = []
    for label, e in format_12_cases(t, every):
        d = decode_ref(e)
        if d is None and is_alias(e):
            d = decode_ref(enc(e[0], int.from_bytes(e[1:], "big") - P))
        cases.append((label, e, _be_y(d) if d is not None else bytes(32)))
    for x, y in tiny_y_points():
        name = "tiny y=%s" % (y if y < EDGE else "p-%d" % (P - y))
        if y + P < TWO256:
            cases.append((name + " hint y+p", enc(2 + ((y + P) & 1), x), (y + P).to_bytes(32, "big")))
            cases.append((name + " right y, other tag", enc(3 - (y & 1), x), y.to_bytes(32, "big")))
    x, y = tiny_y_points()[1]
    for name, v in (("0", 0), ("p", P), ("p+1", P + 1), ("2^256-1", TWO256 - 1), ("y-1", y - 1)):
        cases.append(("tiny y=p-1 hint %s" % name, enc(2 + (v & 1), x), v.to_bytes(32, "big")))
    cases.append(("identity with a hint", bytes(33), (1).to_bytes(32, "big")))
    return cases
