#!/usr/bin/env python3
"""Range proofs of different sizes: ONE mixed call (MixedBatchRangeVerifier.partial_packed -> bpmi_rp_batch_verify_mixed_dev) against what a
user did before it -- a loop of BatchRangeVerifier.partial_wire per class plus ec_sum of the values, on the same build:

  python tools/bench_rp_verify_mixed.py [--reps 7] [--table-bits 12] [--out profiles/r13_rp_verify_mixed.txt]

Shape: proofs of m = 1 / 2 / 4 / 8 / 16 values of 64 bits (AggregNIRangeProver-shaped: over the first 64 m of 1 024 generators), DISTINCT,
wire format 2, proved on the device by BatchRangeProver; 2 048 / 1 024 / 512 / 256 / 256 of them (2^12), and a second line with 64 per class.
Both paths get the same packed inputs (commitments packed, one bytes object of proofs with offsets per class) so that neither pays Python
work per proof.  The two alternate in the same process after a warm-up of both; medians of --reps with min and max.  Then, in a run of its
own with bpmi_profile on, the device time of the preparation stages and of the MSM stages, for the mixed call and summed over the loop.
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
MS = (1, 2, 4, 8, 16)
PREP_STAGES = ("rp_prepare", "rp_elements", "ec_decompress")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--table-bits", type=int, default=12)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import bulletproofs_amd  # noqa: F401
    from bulletproofs_amd.ec import secp256k1
    from bulletproofs_amd.engine import default_engine
    from bulletproofs_amd.rangeproofs import BatchRangeVerifier, MixedBatchRangeVerifier
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
        """(packed commitments, proofs as one bytes object, offsets as a C array) of `count` distinct proofs of m values"""
        tag = b"m%d-" % m
        vs = b"".join(hashlib.sha256(tag + b"v%d" % j).digest()[:8] + bytes(24) for j in range(count * m))
        gammas = b"".join((int.from_bytes(hashlib.sha256(tag + b"gamma%d" % j).digest(), "big") % Q).to_bytes(32, "little") for j in range(count * m))
        bp = BatchRangeProver(bits, g, h, gs[:bits * m], hs[:bits * m], u, m=m, wire_format=2)
        packed, off = bp.prove_wire_packed(vs, gammas, [tag + b"seed%d" % j for j in range(count)])
        vb = bp.commit_packed(vs, gammas)
        bp.close()
        return bytes(vb), bytes(packed), (ctypes.c_uint64 * len(off))(*off)

    def stage_ms(prof):
        prep = sum(ms for name, (ms, _) in prof.items() if any(name.startswith(p) for p in PREP_STAGES))
        rest = sum(ms for name, (ms, _) in prof.items() if not any(name.startswith(p) for p in PREP_STAGES))
        return prep, rest

    mv = MixedBatchRangeVerifier(g, h, gs, hs, u)
    per_class = {m: BatchRangeVerifier(g, h, gs[:bits * m], hs[:bits * m], u) for m in MS}
    for counts in ((2048, 1024, 512, 256, 256), (64,) * 5):
        data = {m: prove(m, c) for m, c in zip(MS, counts)}
        classes = [(bits * m, data[m][0], data[m][1], data[m][2]) for m in MS]

        def mixed():
            return mv.partial_packed(classes)

        def loop():
            vals = [per_class[m].partial_wire(data[m][0], data[m][1], data[m][2]) for m in MS]
            return eng.ec_sum_bytes(b"".join(vals), len(vals))

        assert mixed() == ZERO and loop() == ZERO                # warm-up of both: buffers, workspaces
        mixed(), loop()
        tm, tl = [], []
        for _ in range(args.reps):                               # alternating
            t0 = time.perf_counter()
            a = mixed()
            t1 = time.perf_counter()
            b = loop()
            t2 = time.perf_counter()
            assert a == ZERO and b == ZERO
            tm.append(1e3 * (t1 - t0))
            tl.append(1e3 * (t2 - t1))
        say("proofs per class (m = 1 2 4 8 16): %s = %d proofs, wire format 2, %d alternating repetitions" % (" ".join(map(str, counts)), sum(counts), args.reps))
        say("  mixed call            median %8.3f ms   min %8.3f   max %8.3f" % (statistics.median(tm), min(tm), max(tm)))
        say("  loop over the classes median %8.3f ms   min %8.3f   max %8.3f" % (statistics.median(tl), min(tl), max(tl)))
        # device time by stage, a run of its own
        eng.profile(True)
        for name, f in (("mixed call", mixed), ("loop", loop)):
            eng.profile_reset()
            f()
            prof = eng.profile_read()
            prep, rest = stage_ms(prof)
            say("  %-10s device ms: preparation stages %7.3f   MSM and the rest %7.3f   (%s)" % (
                name, prep, rest, ", ".join("%s %.3f/%d" % (k, v[0], v[1]) for k, v in prof.items() if v[1])))
        eng.profile(False)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    mv.release()
    for bv in per_class.values():
        bv.release()


if __name__ == "__main__":
    main()
