"""What the hash-to-curve tests compare with (tests/test_h2c_host_cpu.py, tests/test_gpu_hash_to_curve.py): the oracle's elliptic_hash,
computed once per process, and the counter it stopped at -- the oracle returns the point of the FIRST candidate that succeeds, so its
counter is the one whose SHA-256 is the point's x."""
import functools
import hashlib
from itertools import count

from oracle import bp_ref as R

P = 2**256 - 2**32 - 977
IDENTITY = bytes(64)


def wire(pt):
    return pt.x.to_bytes(32, "little") + pt.y.to_bytes(32, "little")


def oracle_one(msg):
    """(64 wire bytes, tries) of oracle.bp_ref.elliptic_hash(msg)"""
    pt = R.elliptic_hash(msg)
    for c in count(1):
        if int.from_bytes(hashlib.sha256(b"%d" % c + msg).digest(), "big") == pt.x:
            return wire(pt), c


@functools.lru_cache(maxsize=None)
def oracle_range(tail, lo, hi):
    """([wire bytes], [tries]) of the messages str(i) || tail, i in [lo, hi)"""
    both = [oracle_one(b"%d" % i + tail) for i in range(lo, hi)]
    return [b for b, _ in both], [t for _, t in both]


def gs_set():
    """the 4 096 messages str(i) || b"gs": mean tries 2.008, the largest 13 (i = 1616)"""
    return oracle_range(b"gs", 0, 4096)
