#!/usr/bin/env python3
"""Batch verification of PACKED inner-product proofs of DIFFERENT lengths in one native call
(MixedBatchInnerProductVerifier.verify_packed2, bpmi_ipa_verify_batch_packed_mixed_dev) against what the same build offers beside it, on
one GPU:

  python tools/bench_ipa_verify_packed_mixed.py [--shapes NAME ...] [--distinct 4] [--reps 9] [--out profiles/r17_ipa_verify_packed_mixed.txt]

A shape is a list of (proofs, log2 elements) classes over the prefixes of ONE generator list (the five compositions of
tools/bench_ipa_batch_mixed.py).  Per class `distinct` proofs are made once, packed, and cycled.  One process; after a warm-up of every
path, `reps` ALTERNATING timed calls of each, every one ending in a synchronisation:
  packed mixed   verify_packed2 over the list of classes: ONE native call
  (a) per length one BatchInnerProductVerifier.verify_packed2 per class over that class's prefix (bpmi_ipa_verify_batch_packed_dev), then
                 bpmi_ec_sum of the classes' 64-byte results
  (b) objects    MixedBatchInnerProductVerifier.add for every proof (transcript re-hash on the host), then verify()
The device columns are the stage timers of bpmi_profile in a run of their own: rp_prepare holds the preparation kernels (transposes,
roles, finish), sc_fold the three s-vector kernels, msm the stages of the MSM.  No threshold: the file states what was measured, with
the spread (min .. max) of every median."""
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
    le32 = lambda v: (int(getattr(v, "x", v)) % Q).to_bytes(32, "little")

    def class_of(k):
        """(generators of the prefix, `distinct` proofs over it as objects, and the same proofs as packed rows)"""
        if k not in made:
            n = 1 << k
            g, h = PackedPoints([None] * n, gb[: 64 * n]), PackedPoints([None] * n, hb[: 64 * n])      # the wire form is all that is read
            proofs, rows = [], []
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
                rows.append((u.to_le64(), Pt.to_le64(), le32(a) + le32(b), b"".join(le32(x) for x in xs), b"".join(p.to_le64() for p in Ls + Rs), bytes(tr.digest)))
            made[k] = (g, h, proofs, rows)
        return made[k]

    def packed_class(count, rows):
        """The argument tuple of verify_packed2 for `count` proofs cycling over the rows"""
        pick = [rows[i % len(rows)] for i in range(count)]
        return tuple(b"".join(r[f] for r in pick) for f in range(5)) + ([r[5] for r in pick],)

    class Keeping:
        """the engine, keeping the 64-byte result of every per-class call"""
        def __init__(self):
            self.outs = []

        def __getattr__(self, name):
            return getattr(eng, name)

        def ipa_verify_batch_packed_dev(self, *a, **kw):
            out, status = eng.ipa_verify_batch_packed_dev(*a, **kw)
            self.outs.append(out)
            return out, status

    def device_ms(f):
        """(rp_prepare, sc_fold, the MSM's stages, everything) of one run of f, in ms"""
        eng.profile(True)
        eng.profile_reset()
        f()
        stages = {k: v[0] for k, v in eng.profile_read().items() if v[1]}
        eng.profile(False)
        return stages.get("rp_prepare", 0.0), stages.get("sc_fold", 0.0), sum(ms for k, ms in stages.items() if k.startswith("msm_")), sum(stages.values())

    def spread(ts):
        return "%9.3f (%.3f .. %.3f)" % (1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts))

    say("one process, one GPU; median (min .. max) of %d alternating warm calls, ms; %d distinct proofs per length, cycled" % (args.reps, args.distinct))
    gtop, htop = PackedPoints([None] * N, gb), PackedPoints([None] * N, hb)
    for name, classes in shapes:
        data = [(count, k) + class_of(k) for count, k in classes]
        packed = [packed_class(count, rows) for count, k, g, h, proofs, rows in data]
        mv = MixedBatchInnerProductVerifier(gtop, htop, engine=eng)
        keep = Keeping()
        bvs = []
        for count, k, g, h, proofs, rows in data:
            bvs.append(BatchInnerProductVerifier(g, h, engine=eng))
            bvs[-1].engine = keep

        def packed_mixed():
            assert mv.verify_packed2(packed) is True

        def packed_loop():
            keep.outs = []
            for bv, cls in zip(bvs, packed):
                assert bv.verify_packed2(*cls) is True
            assert eng.ec_sum_bytes(b"".join(keep.outs), len(keep.outs)) == bytes(64)

        def objects():
            mv.reset()
            for count, k, g, h, proofs, rows in data:
                for i in range(count):
                    mv.add(*proofs[i % args.distinct])
            assert mv.verify() is True

        def timed(f):
            t0 = time.perf_counter()
            f()
            eng.sync()
            return time.perf_counter() - t0

        paths = (("mixed", packed_mixed), ("loop", packed_loop), ("objects", objects))
        for _, f in paths:                            # warm: staging buffers, workspaces
            timed(f)
        t = {key: [] for key, _ in paths}
        for _ in range(args.reps):
            for key, f in paths:
                t[key].append(timed(f))
        dm, dl = device_ms(packed_mixed), device_ms(packed_loop)
        med = {key: statistics.median(v) for key, v in t.items()}
        say("%s: %s" % (name, " + ".join("%d x 2^%d" % c for c in classes)))
        say("    packed mixed (one call)   %s" % spread(t["mixed"]))
        say("    (a) packed, per length    %s   ratio (a) / mixed %.2f" % (spread(t["loop"]), med["loop"] / med["mixed"]))
        say("    (b) objects, add+verify   %s   ratio (b) / mixed %.2f" % (spread(t["objects"]), med["objects"] / med["mixed"]))
        say("    device   mixed  rp_prepare %.3f sc_fold %.3f msm %.3f all %.3f" % dm)
        say("             (a)    rp_prepare %.3f sc_fold %.3f msm %.3f all %.3f   (summed over the %d calls)" % (dl + (len(classes),)))
        if med["mixed"] >= med["loop"]:
            say("    the mixed call is NOT faster than (a), the per-length loop of packed calls, here")
        if med["mixed"] >= med["objects"]:
            say("    the mixed call is NOT faster than (b), the object path, here")
        mv.release()
        for bv in bvs:
            bv.release()
    say("(rp_prepare: k_ipap_transpose per class and round, k_ipap_roles_mixed per round, k_ipap_finish_mixed in the mixed call; k_ipap_transpose,")
    say(" k_ipap_roles, k_ipap_finish per class in (a).  sc_fold: the three mixed s-vector kernels / the three per-class ones)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
