"""BPIP2: a wire format for Protocol-2 inner-product proofs (range proofs: rangeproofs/codec.py).  The
reference never serialises a proof, and the packed arrays of BatchInnerProductProver are this library's own layout, which says
everything two or three times: the points as 64-byte rows and as base64 items of the transcript, the challenges as rows and in
decimal.  One proof of n = 2^k elements is one blob (integers big-endian):
  "BPIP2" | k (1 B)                                   k <= 22
  a | b | xs[0..k)                                    (2 + k) x 32 B
  Ls[0..k) Rs[0..k)                                   2k x 33 B SEC1 compressed; the identity = 33 zero bytes
  start_transcript (4 B)
  prefix_len (4 B) | prefix                           the transcript's bytes before item `start_transcript`
78 + 98 k + prefix_len bytes (0.67 KB at n = 64; the packed form is 2.04 KB).  The blob stands for the proof whose transcript is
  prefix || for each round j:  b64(L_j) "&" b64(R_j) "&" str(x_j) "&"
which is what FastNIProver2 writes (src/innerproduct/inner_product_prover.py:94-110 over src/utils/transcript.py:13-29; the prefix
is "&" plus its `transcript` argument).  ONLY such a proof has a wire form: `proof2_to_bytes` raises ValueError for a transcript
with fewer than `start_transcript` "&", or with anything but the canonical rounds behind the prefix -- trailing text included,
although Verifier2 never looks behind the last round (inner_product_verifier.py:104-125) and accepts such a proof.

The functions on single proofs are pure Python; `wire_from_packed` / `packed_from_wire` go through the native host code
(csrc/ipa_wire_host.hpp), and BatchInnerProductVerifier.verify_wire2 hands the bytes to ONE native call that expands them in device
memory (csrc/ipa_wire_kernels.hpp)."""
import ctypes
from base64 import b64encode

from .. import _native
from ..ec import Point, secp256k1
from ..utils.utils import ModP, bytes_to_point, point_to_bytes
from .inner_product_verifier import Proof2

MAGIC = b"BPIP2"
K_MAX = 22
MAX_TRANSCRIPT = 1 << 17
Q = secp256k1.q


def wire_bytes(k, prefix_len):
    """Length of the blob of a proof of 2^k elements."""
    return 78 + 98 * k + prefix_len


def _pt33(P):
    b = point_to_bytes(P)
    return b if len(b) == 33 else bytes(33)


def _rounds_text(xs, comps_l, comps_r):
    item = lambda c: b64encode(c if any(c) else b"\x00")
    return b"".join(item(l) + b"&" + item(r) + b"&" + str(x).encode() + b"&" for x, l, r in zip(xs, comps_l, comps_r))


def proof2_to_bytes(proof) -> bytes:
    """The blob of a Proof2.  ValueError: the proof has no wire form (see the module text)."""
    k = len(proof.xs)
    if k > K_MAX or len(proof.Ls) != k or len(proof.Rs) != k:
        raise ValueError("a Proof2 of k <= 22 rounds with k points in Ls and in Rs")
    scalars = [int(proof.a.x), int(proof.b.x)] + [int(x.x) for x in proof.xs]
    if any(not 0 <= v < Q for v in scalars):
        raise ValueError("a scalar is not below q")
    start, tr = int(proof.start_transcript), bytes(proof.transcript)
    if start < 0 or tr.count(b"&") < start or len(tr) > MAX_TRANSCRIPT:
        raise ValueError("the transcript has fewer than start_transcript '&' (or more than 2^17 bytes)")
    cut = 0
    for _ in range(start):
        cut = tr.index(b"&", cut) + 1
    ls, rs = [_pt33(P) for P in proof.Ls], [_pt33(P) for P in proof.Rs]
    if tr[cut:] != _rounds_text(scalars[2:], ls, rs):
        raise ValueError("behind item start_transcript the transcript is not the canonical text of the rounds")
    return (MAGIC + bytes([k]) + b"".join(v.to_bytes(32, "big") for v in scalars) + b"".join(ls) + b"".join(rs) +
            start.to_bytes(4, "big") + cut.to_bytes(4, "big") + tr[:cut])


def _split(blobs, off=None):
    """A list of blobs, or joined bytes plus offsets -> (joined bytes, offsets)."""
    if off is None:
        blobs = [bytes(b) for b in blobs]
        off, at = [0], 0
        for b in blobs:
            at += len(b)
            off.append(at)
        return b"".join(blobs), off
    return bytes(blobs), [int(o) for o in off]


def proof2_from_bytes(blob) -> Proof2:
    """The Proof2 a blob stands for (pure Python).  ValueError: a malformed blob or a point that does not decode."""
    blob = bytes(blob)
    if len(blob) < 6 or blob[:5] != MAGIC or blob[5] > K_MAX or len(blob) < wire_bytes(blob[5], 0):
        raise ValueError("not a BPIP2 proof")
    k = blob[5]
    pts_at, start_at = 6 + 32 * (2 + k), 6 + 32 * (2 + k) + 66 * k
    scalars = [int.from_bytes(blob[6 + 32 * j: 38 + 32 * j], "big") for j in range(2 + k)]
    start, prefix_len = int.from_bytes(blob[start_at: start_at + 4], "big"), int.from_bytes(blob[start_at + 4: start_at + 8], "big")
    if len(blob) != wire_bytes(k, prefix_len) or any(v >= Q for v in scalars):
        raise ValueError("not a BPIP2 proof")
    comps = [blob[pts_at + 33 * j: pts_at + 33 * j + 33] for j in range(2 * k)]
    for c in comps:
        if c[0] == 0 and any(c):
            raise ValueError("not a compressed point")
    pts = [bytes_to_point(c) for c in comps]
    tr = blob[start_at + 8:] + _rounds_text(scalars[2:], comps[:k], comps[k:])
    if len(tr) > MAX_TRANSCRIPT:
        raise ValueError("not a BPIP2 proof")
    return Proof2(ModP(scalars[0], Q), ModP(scalars[1], Q), [ModP(v, Q) for v in scalars[2:]], pts[:k], pts[k:], tr, start)


def proofs2_from_bytes(blobs, engine=None):
    """[Proof2] of a list of blobs.  Pure Python, one square root per point; `engine` is accepted for symmetry with
    rangeproofs.codec.proofs_from_bytes and not used: a batch that is to be VERIFIED never needs the objects (verify_wire2)."""
    return [proof2_from_bytes(b) for b in blobs]


def _k_of(xs, ab):
    count = len(ab) // 64
    if count == 0 or len(ab) != 64 * count or len(xs) % (32 * count):
        raise ValueError("ab: 64 bytes per proof; xs: 32 k bytes per proof")
    return len(xs) // (32 * count), count


def wire_from_packed(ab, xs, lr, transcripts, starts=None):
    """(blobs, off): the packed arrays of prove2_packed (ab, xs, LR, the list of transcripts; starts: one per proof, None = 1) as
    BPIP2 blobs back to back with n_proofs + 1 offsets -- the native host encoder, bpmi_ipa_wire_encode.  ValueError names the
    proofs that have no wire form."""
    if not transcripts:
        return b"", [0]
    k, count = _k_of(xs, ab)
    if len(transcripts) != count or len(lr) != 128 * k * count or (starts is not None and len(starts) != count):
        raise ValueError("one transcript (and start) per proof; LR: 128 k bytes per proof")
    lib = _native.load()
    tr_off = (ctypes.c_uint64 * (count + 1))()
    for i, t in enumerate(transcripts):
        tr_off[i + 1] = tr_off[i] + len(t)
    cap = count * wire_bytes(k, 0) + tr_off[count]
    blobs, off, status = ctypes.create_string_buffer(cap), (ctypes.c_uint64 * (count + 1))(), ctypes.create_string_buffer(count)
    st = None if starts is None else (ctypes.c_uint32 * count)(*[int(s) for s in starts])
    rc = lib.bpmi_ipa_wire_encode(k, 2, count, bytes(ab), bytes(xs) if k else None, bytes(lr) if k else None, b"".join(transcripts), tr_off, st,
                                  blobs, cap, off, status)
    if rc:
        raise ValueError((lib.bpmi_last_error(None) or b"bpmi_ipa_wire_encode failed").decode())
    bad = [i for i, s in enumerate(status.raw[:count]) if s]
    if bad:
        raise ValueError("no wire form (a transcript that is not prefix + canonical rounds, a scalar >= q, a point off the curve): proofs %s" % bad[:16])
    return blobs.raw[: off[count]], list(off)


def packed_from_wire(blobs, off=None, k=None):
    """(ab, xs, lr, transcripts, starts, status): the packed arrays a batch of blobs (a list, or joined bytes plus offsets) stands
    for, by the native host twin bpmi_ipa_wire_expand; status[i] = bit 0: malformed, bit 1: a point that does not decode (such a
    proof or point has zero rows).  k: the rounds of the batch (None: the k byte of the first blob)."""
    data, off = _split(blobs, off)
    count = len(off) - 1
    if count == 0:
        return b"", b"", b"", [], [], b""
    if k is None:
        k = data[off[0] + 5] if off[1] - off[0] >= 6 else 0
    lib = _native.load()
    offs = (ctypes.c_uint64 * (count + 1))(*off)
    cap = max(sum(max(off[i + 1] - off[i] - wire_bytes(k, 0), 0) for i in range(count)) + 169 * k * count, 1)
    ab, xs, lr = ctypes.create_string_buffer(64 * count), ctypes.create_string_buffer(max(32 * k * count, 1)), ctypes.create_string_buffer(max(128 * k * count, 1))
    tr, tr_off, start, status = ctypes.create_string_buffer(cap), (ctypes.c_uint64 * (count + 1))(), (ctypes.c_uint32 * count)(), ctypes.create_string_buffer(count)
    rc = lib.bpmi_ipa_wire_expand(k, 2, count, data, offs, ab, xs, lr, tr, cap, tr_off, start, status)
    if rc:
        raise ValueError((lib.bpmi_last_error(None) or b"bpmi_ipa_wire_expand failed").decode())
    raw = tr.raw
    return (ab.raw, xs.raw[: 32 * k * count], lr.raw[: 128 * k * count], [raw[tr_off[i]: tr_off[i + 1]] for i in range(count)], list(start),
            status.raw[:count])
