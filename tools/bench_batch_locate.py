#!/usr/bin/env python3
"""What it costs to NAME the invalid proofs of a batch (BatchRangeVerifier.locate_wire, bpmi_rp_batch_group_values_dev) beside what
it costs to verify it, and beside the recourse there was before -- a bisection in Python over partial_wire:

  python tools/bench_batch_locate.py [--log-batch 14] [--group 0] [--reps 5] [--out profiles/r07_batch_locate.txt]

2^log-batch DISTINCT 64-bit proofs in wire format 2 (proved on the device in one call), commitments packed, one page-locked receive
buffer.  Timed, each as the median of --reps warm calls:
  verify_wire                                   the whole batch, one MSM
  locate_wire, 0 / 1 / 16 wrong commitments     the wrong ones spread over distinct groups
  locate_wire, every group failing              one wrong commitment per group: level 2 is the whole batch, one proof per group
  bisection over partial_wire, 1 / 16 wrong     halves re-uploaded, re-parsed, re-hashed and re-decoded at every level
Not bench.py, and not part of benchlib: nothing here is a headline."""
import argparse
import ctypes
import hashlib
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ZERO = bytes(64)


def bisect_partial_wire(bv, packed_v, blobs):
    """The baseline: the indices of the invalid proofs by halving, every half through partial_wire (a proof that fails its byte-level
    checks makes partial_wire raise: that half is split like one whose value is not the identity)."""
    bad = []

    def value_ok(lo, hi):
        try:
            return bv.partial_wire(packed_v[64 * lo: 64 * hi], blobs[lo:hi]) == ZERO
        except Exception as e:
            if "Proof invalid" not in str(e):
                raise
            return False

    def walk(lo, hi, known_bad):
        if not known_bad and value_ok(lo, hi):
            return True
        if hi - lo == 1:
            bad.append(lo)
            return False
        mid = (lo + hi) // 2
        left_ok = walk(lo, mid, False)
        walk(mid, hi, left_ok)                   # the left half is fine: the right one holds a bad proof, no call needed to know
        return False
    walk(0, len(blobs), False)
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-batch", type=int, default=14)
    ap.add_argument("--group", type=int, default=0, help="level-1 group size of locate_wire (0: its default)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import bulletproofs_amd  # noqa: F401
    from bulletproofs_amd.ec import secp256k1
    from bulletproofs_amd.engine import default_engine
    from bulletproofs_amd.rangeproofs import BatchRangeVerifier
    from bulletproofs_amd.rangeproofs.batch_prover import BatchRangeProver
    from bulletproofs_amd.utils import elliptic_hash
    eng = default_engine()
    Q, n, count = secp256k1.q, 64, 1 << args.log_batch
    gs = [elliptic_hash(str(i).encode() + b"gs") for i in range(n)]
    hs = [elliptic_hash(str(i).encode() + b"hs") for i in range(n)]
    g, h, u = elliptic_hash(b"g"), elliptic_hash(b"h"), elliptic_hash(b"u")
    vs = b"".join(hashlib.sha256(b"v%d" % j).digest()[:8] + bytes(24) for j in range(count))          # 64-bit values, little-endian
    gammas = b"".join((int.from_bytes(hashlib.sha256(b"gamma%d" % j).digest(), "big") % Q).to_bytes(32, "little") for j in range(count))
    bp = BatchRangeProver(n, g, h, gs, hs, u, wire_format=2)
    packed, off = bp.prove_wire_packed(vs, gammas, [b"seed%d" % j for j in range(count)])
    bp.close()
    blobs = [packed[off[i]: off[i + 1]] for i in range(count)]
    # V_i = v_i g + gamma_i h
    vg = eng.ec_mul_batch_bytes(g.to_le64() * count, vs, count)
    gh = eng.ec_mul_batch_bytes(h.to_le64() * count, gammas, count)
    one = (1).to_bytes(32, "little")
    good_v = eng.ec_lincomb2_batch_bytes(vg, gh, one, one, count)
    bv = BatchRangeVerifier(g, h, gs, hs, u)
    group = args.group or bv.default_group()
    ngroups = (count + group - 1) // group
    recv = eng.host_alloc(len(packed))
    recv.view[:] = packed
    offs = (ctypes.c_uint64 * (count + 1))(*off)

    def with_wrong(indices):
        v = bytearray(good_v)
        for i in indices:
            j = (i + 1) % count
            v[64 * i: 64 * i + 64] = good_v[64 * j: 64 * j + 64]
        return bytes(v)

    def spread(k):                                # k wrong commitments in k distinct groups, at varying positions inside them
        step = max(1, ngroups // k)
        return sorted({min(count - 1, (t * step) * group + (7 * t + 3) % group) for t in range(k)})

    def timed(f):
        f()                                       # warm: staging buffers, workspaces
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            r = f()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), r

    lines = ["batch: %d distinct 64-bit proofs, wire format 2; locate_wire level-1 group = %d (%d groups); median of %d warm calls"
             % (count, group, ngroups, args.reps)]

    def report(name, seconds, extra=""):
        lines.append("%-58s %9.3f ms%s" % (name, 1e3 * seconds, extra))
        print(lines[-1], flush=True)

    print(lines[0], flush=True)
    t, ok = timed(lambda: bv.verify_wire(good_v, recv, offs))
    assert ok is True
    report("verify_wire (valid batch)", t, "   %.3g verifies/s" % (count / t))
    for k in (0, 1, 16):
        want = spread(k) if k else []
        v = with_wrong(want)
        t, got = timed(lambda: bv.locate_wire(v, recv, offs, group=group))
        assert got == want, (got, want)
        report("locate_wire, %d wrong commitment(s) in distinct groups" % k, t)
    want = [t_ * group + (5 * t_) % min(group, count - t_ * group) for t_ in range(ngroups)]
    v = with_wrong(want)
    t, got = timed(lambda: bv.locate_wire(v, recv, offs, group=group))
    assert got == want
    report("locate_wire, every group failing (%d wrong)" % len(want), t)
    t, (values, status) = timed(lambda: bv.group_values_wire(good_v, recv, offs, group=group))
    assert values == [ZERO] * ngroups and status == bytes(count)
    report("group_values_wire alone, group = %d" % group, t)
    t, (values, status) = timed(lambda: bv.group_values_wire(good_v, recv, offs, group=1))
    assert values == [ZERO] * count
    report("group_values_wire alone, group = 1 (%d MSMs of %d pairs)" % (count, 3 + 2 * n + 19), t)
    for k in (1, 16):
        want = spread(k)
        v = with_wrong(want)
        t, got = timed(lambda: bisect_partial_wire(bv, v, blobs))
        assert got == want, (got, want)
        report("bisection over partial_wire, %d wrong commitment(s)" % k, t)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    recv.free()
    bv.release()


if __name__ == "__main__":
    main()
