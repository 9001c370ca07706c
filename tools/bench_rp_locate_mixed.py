#!/usr/bin/env python3
"""Naming the invalid proofs of a block of range proofs of DIFFERENT sizes: the two-level plan of MixedBatchRangeVerifier.locate_wire over
bpmi_rp_batch_group_values_mixed_dev (group = None: default_groups, then one call with one proof per group) against the class-by-class
path (group = 0: BatchRangeVerifier.locate_wire per class), on the same build, the same proofs, in the same process, on one GPU:

  python tools/bench_rp_locate_mixed.py [--reps 9] [--table-bits 12] [--out profiles/r20_rp_locate_mixed.txt]

  shape   the block of profiles/r13_rp_verify_mixed.txt: 2 048 / 1 024 / 512 / 256 / 256 DISTINCT proofs of m = 1 / 2 / 4 / 8 / 16 values of
          64 bits over the first 64 m of 1 024 generators, wire format 2, proved on the device by BatchRangeProver; the items in class order
  cases   0, 1 and 16 wrong commitments (a proof's commitments replaced by its neighbour's in the class, spread evenly over the block),
          and one wrong commitment in every level-1 group of every class
  method  per case one warm-up of either path, then `reps` ALTERNATING calls (a) group=None / (b) group=0; median with min and max; both
          must return the expected indices.  Wall = host clock around a call that ends in a synchronisation; both paths do the same
          Python work per item (classes(), packing).  For the valid block also verify_wire

No threshold: the file states what was measured."""
import argparse
import hashlib
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

MS = (1, 2, 4, 8, 16)
COUNTS = (2048, 1024, 512, 256, 256)


def spread(ts):
    return "%9.3f ms (min %.3f max %.3f)" % (1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts))


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--table-bits", type=int, default=12)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import bulletproofs_amd  # noqa: F401
    from bulletproofs_amd.ec import Point, secp256k1
    from bulletproofs_amd.engine import default_engine
    from bulletproofs_amd.rangeproofs import MixedBatchRangeVerifier
    from bulletproofs_amd.rangeproofs.batch_prover import BatchRangeProver
    from bulletproofs_amd.utils import elliptic_hash
    eng = default_engine()
    eng.set_option("prover_table_bits", args.table_bits)
    Q, bits, N = secp256k1.q, 64, 64 * MS[-1]
    gs = [elliptic_hash(str(i).encode() + b"gs") for i in range(N)]
    hs = [elliptic_hash(str(i).encode() + b"hs") for i in range(N)]
    g, h, u = elliptic_hash(b"g"), elliptic_hash(b"h"), elliptic_hash(b"u")
    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def prove(m, count):
        """[(commitments of proof j as Points, wire proof j)] of `count` distinct proofs of m values"""
        tag = b"m%d-" % m
        vs = b"".join(hashlib.sha256(tag + b"v%d" % j).digest()[:8] + bytes(24) for j in range(count * m))
        gammas = b"".join((int.from_bytes(hashlib.sha256(tag + b"gamma%d" % j).digest(), "big") % Q).to_bytes(32, "little") for j in range(count * m))
        bp = BatchRangeProver(bits, g, h, gs[:bits * m], hs[:bits * m], u, m=m, wire_format=2)
        packed, off = bp.prove_wire_packed(vs, gammas, [tag + b"seed%d" % j for j in range(count)])
        vb = bytes(bp.commit_packed(vs, gammas))
        bp.close()
        packed = bytes(packed)
        Vs = [Point.from_le64(vb[64 * i: 64 * i + 64]) for i in range(count * m)]
        return [(Vs[j] if m == 1 else Vs[m * j: m * j + m], packed[off[j]: off[j + 1]]) for j in range(count)]

    made = [prove(m, c) for m, c in zip(MS, COUNTS)]
    first = [sum(COUNTS[:c]) for c in range(len(MS))]
    total = sum(COUNTS)
    mv = MixedBatchRangeVerifier(g, h, gs, hs, u)

    def items_with(bad):
        """the block in class order, the commitments of the global indices `bad` replaced by the next proof's of the class"""
        bad, out = set(bad), []
        for c, cls in enumerate(made):
            out += [(cls[(j + 1) % len(cls)][0], blob) if first[c] + j in bad else (V, blob) for j, (V, blob) in enumerate(cls)]
        return out

    try:
        groups = mv.default_groups([(bits * m, m) for m in MS])
        say("one MI355X; %s proofs of m = %s values of 64 bits = %d proofs, wire format 2, distinct; default_groups %s; per case one warm-up of either path, then %d "
            "alternating calls (a) locate_wire(group=None) / (b) locate_wire(group=0), class by class: median (min max); wall = host clock around a call that ends in a "
            "synchronisation" % (" / ".join(map(str, COUNTS)), " / ".join(map(str, MS)), total, groups, args.reps))
        valid = items_with([])
        assert mv.verify_wire(valid) is True, "the block must verify"
        ts = []
        for _ in range(args.reps):
            t, ok = timed(lambda: mv.verify_wire(valid))
            assert ok is True
            ts.append(t)
        say("    verify_wire over the valid block %s" % spread(ts))
        every = [first[c] + t * grp + grp // 2 for c, grp in enumerate(groups) for t in range(-(-COUNTS[c] // grp))]
        cases = [("0 wrong", []), ("1 wrong", [total // 3]), ("16 wrong", [(total * j) // 16 + 1 for j in range(16)]), ("one wrong in every group (%d)" % len(every), every)]
        for label, bad in cases:
            bad = sorted(set(bad))
            items = items_with(bad)
            paths = (lambda: mv.locate_wire(items, group=None), lambda: mv.locate_wire(items, group=0))
            for f in paths:
                assert f() == bad, label
            tss = ([], [])
            for _ in range(args.reps):
                for f, acc in zip(paths, tss):
                    t, r = timed(f)
                    assert r == bad
                    acc.append(t)
            ma, mb = (statistics.median(x) for x in tss)
            say("    %-30s (a) group=None %s | (b) group=0 %s | b / a %6.2f%s" % (label, spread(tss[0]), spread(tss[1]), mb / ma, "   <- the plan LOSES to class by class" if ma > mb else ""))
    finally:
        mv.release()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
