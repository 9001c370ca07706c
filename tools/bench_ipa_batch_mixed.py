#!/usr/bin/env python3
"""Batch verification of inner-product proofs of DIFFERENT lengths in one call (innerproduct/batch_mixed.py,
bpmi_ipa_verify_batch_mixed_dev) against what the same build offered before: one BatchInnerProductVerifier per length class
(bpmi_ipa_verify_batch_dev over that class's prefix of the generators) and bpmi_ec_sum over the classes' results, on one GPU:

  python tools/bench_ipa_batch_mixed.py [--shapes NAME ...] [--distinct 4] [--reps 9] [--out profiles/r16_ipa_verify_mixed.txt]

A shape is a list of (proofs, log2 elements) classes over the prefixes of ONE generator list.  Per class `distinct` proofs are made
once and cycled.  One process; after a warm-up of both, `reps` ALTERNATING timed calls of each, every one ending in a synchronisation:
  mixed      MixedBatchInnerProductVerifier.add for every proof (transcript re-hash on the host), then verify(): ONE native call
  per class  per class BatchInnerProductVerifier.add for every proof and verify(), then bpmi_ec_sum of the classes' 64-byte results
The transcript re-hash is the same Python work in both; "verify" leaves it out (the proofs stay queued).  The device columns are
the stage timers of bpmi_profile in a run of their own: sc_fold holds the three s-vector kernels, msm the stages of the MSM.
No threshold: the file states what was measured, with the spread (min .. max) of every median."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = {
    "two": [(1, 6), (1, 10)],
    "few": [(4, 6), (4, 8), (4, 10), (4, 16)],
    "one-length": [(256, 10)],
    "service": [(1 << 12, 6), (1 << 10, 8), (256, 10), (16, 16)],
    "long+short": [(1, 20), (1 << 14, 6)],
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import bulletproofs_amd  # noqa: F401
    from bulletproofs_amd.ec import PackedPoints, Point, secp256k1
    from bulletproofs_amd.engine import default_engine
    from bulletproofs_amd.innerproduct import BatchInnerProductVerifier, MixedBatchInnerProductVerifier, Proof2
    from bulletproofs_amd.innerproduct._rounds import run_rounds
    from bulletproofs_amd.utils import ModP, elliptic_hash
    from bulletproofs_amd.utils.transcript import Transcript
    eng = default_engine()
    Q = secp256k1.q
    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def scalars(count, seed):                       # `count` packed scalars below 2^255 < q
        arr = np.random.default_rng(seed).integers(0, 256, size=(count, 32), dtype=np.uint8)
        arr[:, 31] &= 0x7F
        return arr.tobytes()

    shapes = [(name, SHAPES[name]) for name in args.shapes]
    K = max(k for _, classes in shapes for _, k in classes)
    N = 1 << K
    raw = eng.ec_mul_batch_bytes(secp256k1.G.to_le64() * (2 * N), scalars(2 * N, K), 2 * N)
    gb, hb = raw[: 64 * N], raw[64 * N:]
    made = {}

    def class_of(k):
        """(generators of the prefix, `distinct` proofs over it)"""
        if k not in made:
            n = 1 << k
            g, h = PackedPoints([None] * n, gb[: 64 * n]), PackedPoints([None] * n, hb[: 64 * n])      # the wire form is all that is read
            proofs = []
            for j in range(args.distinct):
                u = elliptic_hash(b"u%d-%d" % (k, j))
                ab, bb = scalars(n, 1000 * k + 2 * j), scalars(n, 1000 * k + 2 * j + 1)
                c = int.from_bytes(eng.sc_dot_bytes(ab, bb, n), "little")
                Pt = Point.from_le64(eng.msm_bytes(gb[: 64 * n] + hb[: 64 * n], ab + bb, 2 * n)) + c * u
                st, tr, xs, Ls, Rs = eng.ipa_create(gb[: 64 * n], hb[: 64 * n], ab, bb, n, u.to_le64()), Transcript(), [], [], []
                run_rounds(st, tr, Q, xs, Ls, Rs)
                a, b = st.finish()
                st.close()
                proofs.append((u, Pt, Proof2(ModP(a, Q), ModP(b, Q), xs, Ls, Rs, tr.digest, 1)))
            made[k] = (g, h, proofs)
        return made[k]

    class Keeping:
        """the engine, keeping the 64-byte result of every per-class call"""
        def __init__(self):
            self.outs = []

        def __getattr__(self, name):
            return getattr(eng, name)

        def ipa_verify_batch_dev(self, *a, **kw):
            self.outs.append(eng.ipa_verify_batch_dev(*a, **kw))
            return self.outs[-1]

    def device_ms(f):
        """(sc_fold, the MSM's stages, everything) of one run of f, in ms"""
        eng.profile(True)
        eng.profile_reset()
        f()
        stages = {k: v[0] for k, v in eng.profile_read().items() if v[1]}
        eng.profile(False)
        return stages.get("sc_fold", 0.0), sum(ms for k, ms in stages.items() if k.startswith("msm_")), sum(stages.values())

    def spread(ts):
        return "%9.3f (%.3f .. %.3f)" % (1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts))

    say("one process, one GPU; median (min .. max) of %d alternating warm calls, ms; %d distinct proofs per length, cycled" % (args.reps, args.distinct))
    gtop, htop = PackedPoints([None] * N, gb), PackedPoints([None] * N, hb)
    for name, classes in shapes:
        data = [(count, k) + class_of(k) for count, k in classes]
        mv = MixedBatchInnerProductVerifier(gtop, htop, engine=eng)
        keep = Keeping()
        bvs = []
        for count, k, g, h, proofs in data:
            bvs.append(BatchInnerProductVerifier(g, h, engine=eng))
            bvs[-1].engine = keep

        def mixed_add():
            mv.reset()
            for count, k, g, h, proofs in data:
                for i in range(count):
                    mv.add(*proofs[i % args.distinct])

        def mixed_verify():
            assert mv.verify() is True

        def classes_add():
            for bv, (count, k, g, h, proofs) in zip(bvs, data):
                bv.reset()
                for i in range(count):
                    bv.add(*proofs[i % args.distinct])

        def classes_verify():
            keep.outs = []
            for bv in bvs:
                assert bv.verify() is True
            assert eng.ec_sum_bytes(b"".join(keep.outs), len(keep.outs)) == bytes(64)

        def timed(fs):
            t0 = time.perf_counter()
            for f in fs:
                f()
            eng.sync()
            return time.perf_counter() - t0

        for fs in ((mixed_add, mixed_verify), (classes_add, classes_verify)):          # warm: staging buffers, workspaces
            timed(fs)
        t = {"mixed": [], "classes": [], "mixed verify": [], "classes verify": []}
        for _ in range(args.reps):
            t["mixed"].append(timed((mixed_add, mixed_verify)))
            t["classes"].append(timed((classes_add, classes_verify)))
            t["mixed verify"].append(timed((mixed_verify,)))
            t["classes verify"].append(timed((classes_verify,)))
        dm, dc = device_ms(mixed_verify), device_ms(classes_verify)
        n_top = 1 << max(k for _, k in classes)
        extra = sum(count * (2 * k + 2) for count, k in classes)
        say("%s: %s" % (name, " + ".join("%d x 2^%d" % c for c in classes)))
        say("    add+verify   mixed %s   per class %s   ratio %.2f" % (spread(t["mixed"]), spread(t["classes"]), statistics.median(t["classes"]) / statistics.median(t["mixed"])))
        say("    verify       mixed %s   per class %s   ratio %.2f" % (spread(t["mixed verify"]), spread(t["classes verify"]),
                                                                        statistics.median(t["classes verify"]) / statistics.median(t["mixed verify"])))
        say("    device       mixed sc_fold %.3f msm %.3f all %.3f   per class sc_fold %.3f msm %.3f all %.3f" % (dm + dc))
        say("    MSM pairs    mixed %d   per class %s" % (2 * n_top + extra, " + ".join(str(2 * (1 << k) + count * (2 * k + 2)) for count, k in classes)))
        if statistics.median(t["mixed"]) >= statistics.median(t["classes"]):
            say("    the mixed call is NOT faster than the per-class loop here")
        mv.release()
        for bv in bvs:
            bv.release()
    say("(sc_fold: k_sc_svector_tables_mixed, k_sc_svector_sum_mixed, k_sc_svector_sum_finish_mixed in the mixed call; k_sc_svector_tables_batch,")
    say(" k_sc_svector_sum, k_sc_svector_sum_finish per class in the loop)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
