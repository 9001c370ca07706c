"""Deriving curve points from byte strings ("nothing up my sleeve" generators).

Try-and-increment exactly as the reference does it (/root/reference/src/utils/
elliptic_curve_hash.py:7-23), because the generators are INPUTS of every golden vector: the
counter i = 1, 2, ... is prefixed in decimal, SHA-256 gives the candidate x, the first candidate
below p whose x^3 + ax + b is a square wins, and the parity of MD5(prefix) picks which of the
two square roots is y (root r = rhs^((p+1)/4) when the parity is odd, p - r otherwise).
`elliptic_hash` of ONE message is host integers only: a kernel launch for one point would be slower.  Generator lists -- thousands
to millions of points -- are derived on the device by `elliptic_hash_batch` and `elliptic_hash_range` (bpmi_ec_hash_*,
csrc/h2c_kernels.hpp): the same function, point for point."""
import hashlib
from itertools import count

from ..ec import PackedPoints, Point, mod_sqrt, secp256k1, unpack_points


def _candidates(msg):
    for i in count(1):
        tagged = b"%d" % i + msg
        yield tagged, int.from_bytes(hashlib.sha256(tagged).digest(), "big")


def elliptic_hash(msg: bytes, CURVE=secp256k1):
    p, a, b = CURVE.p, CURVE.a, CURVE.b
    for tagged, x in _candidates(msg):
        if x >= p:
            continue
        root = mod_sqrt((x * x * x + a * x + b) % p, p)[0]
        if not CURVE.is_point_on_curve((x, root)):
            continue                                   # the right-hand side was not a square
        keep_root = int(hashlib.md5(tagged).hexdigest(), 16) & 1
        return Point(x, root if keep_root else p - root, CURVE)


def elliptic_hash_batch(msgs, engine=None):
    """[elliptic_hash(m) for m in msgs], computed on the device -> PackedPoints."""
    from ..engine import default_engine
    msgs = [bytes(m) for m in msgs]
    packed = (engine or default_engine()).ec_hash_batch_bytes(msgs)
    return PackedPoints(unpack_points(packed, len(msgs)), packed)


def elliptic_hash_range(tail, lo, hi, device=False, engine=None):
    """[elliptic_hash(str(i).encode() + tail) for i in range(lo, hi)], computed on the device -> PackedPoints, or with
    device=True a DeviceBuffer of hi - lo points that never visit the host: ready to be d_g / d_h."""
    from ..engine import default_engine
    eng = engine or default_engine()
    if device:
        return eng.ec_hash_range_dev(tail, lo, hi)
    packed = eng.ec_hash_range_bytes(tail, lo, hi)
    return PackedPoints(unpack_points(packed, hi - lo), packed)
