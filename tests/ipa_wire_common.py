"""What the tests of the wire format BPIP2 share (tests/test_ipa_wire_cpu.py, tests/test_gpu_ipa_wire.py): the golden proofs of
tests/golden/ipa.json as packed rows and as Proof2 objects, the layout of a blob, and the table of malformed blobs with the status
bit each must give.  The expected values come from the format's definition (include/bpmi.h) and from oracle/ec.py, never from the
code under test."""
import json
import os

from oracle.ec import mod_sqrt, secp256k1

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q, P_FIELD = secp256k1.q, secp256k1.p


def golden_cases():
    with open(os.path.join(REPO, "tests", "golden", "ipa.json")) as f:
        return json.load(f)["cases"]


def golden_proofs(case):
    """The two Protocol-2 proofs of a golden case as dicts: the plain one (start 1, prefix "&") and the one inside proof1 (start 3)."""
    return [("proof2", case["proof2"]), ("proof1.proof2", case["proof1"]["proof2"])]


def le64(xy):
    x, y = int(xy[0], 16), int(xy[1], 16)
    return x.to_bytes(32, "little") + y.to_bytes(32, "little")


def packed_of(w2):
    """(k, ab, xs, lr, transcript, start) of a golden Proof2 dict in the packed layout of include/bpmi.h."""
    sc = lambda h: int(h, 16).to_bytes(32, "little")
    k = len(w2["xs"])
    return (k, sc(w2["a"]) + sc(w2["b"]), b"".join(sc(x) for x in w2["xs"]), b"".join(le64(p) for p in w2["Ls"] + w2["Rs"]),
            w2["transcript"].encode(), w2["start_transcript"])


def proof2_of(w2):
    """The package's Proof2 with a golden dict's fields."""
    from bulletproofs_amd.ec import Point, secp256k1 as curve
    from bulletproofs_amd.innerproduct.inner_product_verifier import Proof2
    from bulletproofs_amd.utils import ModP

    def pt(xy):
        x, y = int(xy[0], 16), int(xy[1], 16)
        return Point.IDENTITY_ELEMENT if x == 0 and y == 0 else Point(x, y, curve)
    sc = lambda h: ModP(int(h, 16), Q)
    return Proof2(sc(w2["a"]), sc(w2["b"]), [sc(x) for x in w2["xs"]], [pt(p) for p in w2["Ls"]], [pt(p) for p in w2["Rs"]], w2["transcript"].encode(),
                  w2["start_transcript"])


# ---- the layout of a blob (include/bpmi.h) ----
def fixed_bytes(k):
    return 78 + 98 * k


def scalar_at(j):
    """Byte offset of scalar j: a, b, x_0 .."""
    return 6 + 32 * j


def point_at(k, j):
    """Byte offset of point j: L_0 .. L_(k-1) R_0 .. R_(k-1)."""
    return 6 + 32 * (2 + k) + 33 * j


def start_at(k):
    return 6 + 32 * (2 + k) + 66 * k


def blob_of(k, a, b, xs, comps, start, prefix):
    """A blob from integers, 33-byte encodings and a prefix: the format written out by hand."""
    assert len(xs) == k and len(comps) == 2 * k
    return (b"BPIP2" + bytes([k]) + b"".join(v.to_bytes(32, "big") for v in [a, b] + list(xs)) + b"".join(comps) + start.to_bytes(4, "big") +
            len(prefix).to_bytes(4, "big") + prefix)


def with_bytes(blob, at, new):
    return blob[:at] + new + blob[at + len(new):]


def with_prefix(blob, k, prefix, start=None):
    """The blob with another prefix (and start): well formed, though no longer a valid proof."""
    s = blob[start_at(k): start_at(k) + 4] if start is None else start.to_bytes(4, "big")
    return blob[:start_at(k)] + s + len(prefix).to_bytes(4, "big") + prefix


def x_without_root():
    """An x below p with x^3 + 7 a non-residue, found with the oracle's square root."""
    x = 5
    while True:
        rhs = (x * x * x + 7) % P_FIELD
        if pow(rhs, (P_FIELD - 1) // 2, P_FIELD) == P_FIELD - 1:
            assert not [r for r in mod_sqrt(rhs, P_FIELD) if r * r % P_FIELD == rhs]
            return x
        x += 1


def malformed_table(k):
    """[(name, mutation of a valid blob of k >= 1 rounds, status bit)]: each of the issue's malformed inputs."""
    p0 = point_at(k, 0)
    return [
        ("bad_magic", lambda b: b"BPIP3" + b[5:], 1),
        ("wrong_k_byte", lambda b: with_bytes(b, 5, bytes([k + 1])), 1),
        ("one_short", lambda b: b[:-1], 1),
        ("one_long", lambda b: b + b"&", 1),
        ("tag_4", lambda b: with_bytes(b, p0, b"\x04"), 2),
        ("tag_0_x_1", lambda b: with_bytes(b, p0, bytes(32) + b"\x01"), 2),
        ("x_is_p", lambda b: with_bytes(b, p0 + 1, P_FIELD.to_bytes(32, "big")), 2),
        ("x_without_y", lambda b: with_bytes(b, p0 + 1, x_without_root().to_bytes(32, "big")), 2),
    ]


def decompress_oracle(comp):
    """64 bytes little-endian of a 33-byte encoding by the oracle's arithmetic (zero: the identity); None: it does not decode."""
    x = int.from_bytes(comp[1:], "big")
    if comp[0] == 0:
        return bytes(64) if x == 0 else None
    if comp[0] not in (2, 3) or x >= P_FIELD:
        return None
    rhs = (x * x * x + 7) % P_FIELD
    roots = [r for r in mod_sqrt(rhs, P_FIELD) if r * r % P_FIELD == rhs]
    if not roots:
        return None
    y = roots[0] if (roots[0] & 1) == (comp[0] & 1) else P_FIELD - roots[0]
    return x.to_bytes(32, "little") + y.to_bytes(32, "little")
