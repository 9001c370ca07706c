#!/usr/bin/env python3
"""Batch verification of inner-product proofs over shared generators (innerproduct/batch.py, bpmi_ipa_verify_batch_dev) against
the loop of Verifier2.verify_dev over the same proofs on the same build, on one GPU:

  python tools/bench_ipa_batch_verify.py [--log-n 12 16 20] [--batch 1 4 16 64] [--distinct 4] [--reps 5] [--out profiles/r08_ipa_batch_verify.txt]

For every n and batch size B: `distinct` proofs are made once (random a, b, u; the raw prover state, no Python lists of n objects)
and cycled to fill the batch.  Timed, as the median of `reps` warm runs ending in a synchronisation:
  batch add+verify   BatchInnerProductVerifier.add (transcript re-hash on the host) for every proof, then verify()
  batch verify       verify() alone: packing, ONE native call
  loop               Verifier2.verify_dev per proof (transcript re-hash, one s-vector launch and one MSM each)
  loop, checked      the same with the transcripts checked beforehand
and the device time of each (the stage timers of bpmi_profile, in a run of its own).  The loop's code is what it was before
the batch verifier existed, so its time is the figure to compare against.  No threshold: the file states what was measured."""
import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[12, 16, 20])
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import bulletproofs_amd  # noqa: F401
    from bulletproofs_amd.ec import PackedPoints, Point, secp256k1
    from bulletproofs_amd.engine import default_engine
    from bulletproofs_amd.innerproduct import BatchInnerProductVerifier, Proof2, Verifier2
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

    def timed(f):
        f()                                         # warm: staging buffers, workspaces
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            f()
            eng.sync()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    def device_ms(f):
        """(total of the stage timers, the stages) of one run of f"""
        eng.profile(True)
        eng.profile_reset()
        f()
        stages = {k: v for k, v in eng.profile_read().items() if v[1]}
        eng.profile(False)
        return sum(ms for ms, _ in stages.values()), stages

    say("median of %d warm runs, one GPU; %d distinct proofs per n, cycled; times in ms; ratio = loop / batch add+verify" % (args.reps, args.distinct))
    say("%8s %4s | %12s %10s %10s | %10s %10s %10s | %6s | %s" % ("n", "B", "add+verify", "verify", "device", "loop", "checked", "device", "ratio", "MSM pairs: batch / loop"))
    for log_n in args.log_n:
        n = 1 << log_n
        raw = eng.ec_mul_batch_bytes(secp256k1.G.to_le64() * (2 * n), scalars(2 * n, log_n), 2 * n)
        gb, hb = raw[: 64 * n], raw[64 * n:]
        g, h = PackedPoints([None] * n, gb), PackedPoints([None] * n, hb)          # the wire form is all that is read
        d_g, d_h = g.device(eng), h.device(eng)
        proofs = []
        for j in range(args.distinct):
            u = elliptic_hash(b"u%d" % j)
            ab, bb = scalars(n, 1000 * log_n + 2 * j), scalars(n, 1000 * log_n + 2 * j + 1)
            c = int.from_bytes(eng.sc_dot_bytes(ab, bb, n), "little")
            Pt = Point.from_le64(eng.msm_bytes(gb + hb, ab + bb, 2 * n)) + c * u
            st, tr, xs, Ls, Rs = eng.ipa_create(gb, hb, ab, bb, n, u.to_le64()), Transcript(), [], [], []
            run_rounds(st, tr, Q, xs, Ls, Rs)
            a, b = st.finish()
            st.close()
            proofs.append((u, Pt, Proof2(ModP(a, Q), ModP(b, Q), xs, Ls, Rs, tr.digest, 1)))
        for B in args.batch:
            batch = [proofs[i % args.distinct] for i in range(B)]
            bv = BatchInnerProductVerifier(g, h, engine=eng)

            def add_and_verify():
                bv.reset()
                for u, Pt, pr in batch:
                    bv.add(u, Pt, pr)
                assert bv.verify() is True

            def loop(checked):
                for u, Pt, pr in batch:
                    assert Verifier2(None, None, u, Pt, pr).verify_dev(d_g, d_h, n, engine=eng, _transcript_checked=checked) is True

            t_all = timed(add_and_verify)
            t_verify = timed(lambda: bv.verify())
            t_loop, t_checked = timed(lambda: loop(False)), timed(lambda: loop(True))
            dev_batch, st_batch = device_ms(lambda: bv.verify())
            dev_loop, st_loop = device_ms(lambda: loop(True))
            say("%8d %4d | %12.3f %10.3f %10.3f | %10.3f %10.3f %10.3f | %6.2f | %d / %d x %d" %
                (n, B, 1e3 * t_all, 1e3 * t_verify, dev_batch, 1e3 * t_loop, 1e3 * t_checked, dev_loop, t_loop / t_all,
                 2 * n + B * (2 * log_n + 2), B, 2 * n + 2 * log_n + 2))
            if (log_n, B) == (16, 16) or (t_all >= t_loop and B > 1):
                if t_all >= t_loop:
                    say("    the batch is NOT faster than the loop here")
                say("    stages, batch: " + ", ".join("%s %.3f ms / %d" % (k, ms, c) for k, (ms, c) in st_batch.items()))
                say("    stages, loop:  " + ", ".join("%s %.3f ms / %d" % (k, ms, c) for k, (ms, c) in st_loop.items()))
            bv.release()
        g.release()
        h.release()
    say("(stage sc_fold holds the s-vector kernels: k_sc_svector_tables_batch, k_sc_svector_sum, k_sc_svector_sum_finish in the batch;")
    say(" k_sc_svector_tables, k_sc_svector per proof in the loop)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
