#!/usr/bin/env python3
"""The batch verifier of PACKED inner-product proofs (BatchInnerProductVerifier.verify_packed2, bpmi_ipa_verify_batch_packed_dev) against
the object path of the same build -- BatchInnerProductVerifier.add per proof plus verify() -- on the same proofs, on one GPU:

  python tools/bench_ipa_verify_packed.py [--reps 5] [--step-timeout 400] [--out profiles/r12_ipa_verify_packed.txt]

Every step runs in a process of its own under `--step-timeout` seconds; a step that fails or runs out of time ends the run (nothing
more is started on the GPU behind it).  Within a step the generators, witnesses, statements (one batched MSM) and proofs are made
once, everything that is timed runs ONCE as a warm-up, then the median of `reps` runs is reported.

  shapes  (n, proofs) = (64, 2^14), (256, 2^12), (1024, 2^10), (64, 16), (64, 1) from the batch prover (8-bit tables: the proofs
          do not depend on them), and (2^16, 64) with proofs from FastNIProver2; Protocol 2, every proof from the empty transcript
  packed wall     one verify_packed2 call over packed bytes, host clock (the call ends in a synchronisation)
  packed device   the same call under the engine's stage events (a run of its own): preparation kernels (transpose, roles,
                  finish) | s-vector sum (tables, sum, finish) | the MSM's stages
  object wall     add(u, P, proof) per proof + verify() over the first min(proofs, OBJ_MAX) proofs, timed with the Proof2 / Point
                  objects built beforehand ("objects ready") and with their construction from the packed bytes inside the timed
                  region ("from bytes"); the packed call is timed over the same subset beside it

No threshold: the file states what was measured."""
import argparse
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [(64, 1 << 14), (256, 1 << 12), (1024, 1 << 10), (64, 16), (64, 1), (1 << 16, 64)]
OBJ_MAX = 1024
Q = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


def scalars(count, seed):
    """`count` packed scalars below 2^255 < q"""
    import numpy as np
    arr = np.random.default_rng(seed).integers(0, 256, size=(count, 32), dtype=np.uint8)
    arr[:, 31] &= 0x7F
    return arr.tobytes()


def median_of(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts), r


def step_shape(n, count, reps):
    import bulletproofs_amd  # noqa: F401
    from bulletproofs_amd.ec import PackedPoints, PackedScalars, Point, secp256k1
    from bulletproofs_amd.engine import default_engine
    from bulletproofs_amd.innerproduct import BatchInnerProductProver, BatchInnerProductVerifier, FastNIProver2
    eng = default_engine()
    k = n.bit_length() - 1
    cnt = 2 * n + 1
    raw = eng.ec_mul_batch_bytes(secp256k1.G.to_le64() * cnt, scalars(cnt, n), cnt)
    g, h = PackedPoints([None] * n, raw[: 64 * n]), PackedPoints([None] * n, raw[64 * n: 128 * n])
    u = Point.from_le64(raw[128 * n:])
    ab, bb = scalars(count * n, 7 * n + count), scalars(count * n, 11 * n + count)
    # the statements P_p = <a_p, g> + <b_p, h> + <a_p, b_p> u: one MSM per proof over [g | h | u]
    Ps = b""
    for p in range(count):
        a_row, b_row = ab[32 * n * p: 32 * n * (p + 1)], bb[32 * n * p: 32 * n * (p + 1)]
        Ps += eng.msm_bytes(raw, a_row + b_row + eng.sc_dot_bytes(a_row, b_row, n), cnt)
    us = u.to_le64() * count
    if n <= 1024:
        eng.set_option("prover_table_bits", 8)
        bp = BatchInnerProductProver(g, h, u, engine=eng)
        try:
            pab, pxs, plr, trs = bp.prove2_packed(ab, bb)
        finally:
            bp.close()
            eng.set_option("prover_table_bits", 0)
        source = "batch prover"
    else:
        pab, pxs, plr, trs = b"", b"", b"", []
        for p in range(count):
            a = PackedScalars.from_bytes(ab[32 * n * p: 32 * n * (p + 1)])
            b = PackedScalars.from_bytes(bb[32 * n * p: 32 * n * (p + 1)])
            pr = FastNIProver2(g, h, u, None, a, b, secp256k1).prove()
            pab += (pr.a.x % Q).to_bytes(32, "little") + (pr.b.x % Q).to_bytes(32, "little")
            pxs += b"".join((x.x % Q).to_bytes(32, "little") for x in pr.xs)
            plr += b"".join(pt.to_le64() for pt in pr.Ls + pr.Rs)
            trs.append(pr.transcript)
        source = "FastNIProver2"
    bv = BatchInnerProductVerifier(g, h, engine=eng)
    try:
        packed = lambda c: bv.verify_packed2(us[: 64 * c], Ps[: 64 * c], pab[: 64 * c], pxs[: 32 * k * c], plr[: 128 * k * c], trs[:c])
        t_new, lo, hi, verdict = median_of(lambda: packed(count), reps)
        assert verdict is True, "the batch must verify"
        eng.profile(True)
        eng.profile_reset()
        packed(count)
        prof = eng.profile_read()
        eng.profile(False)
        prep, svec = prof["rp_prepare"][0], prof["sc_fold"][0]
        msm = sum(ms for name, (ms, _) in prof.items() if name.startswith("msm_"))
        other = sum(ms for name, (ms, _) in prof.items()) - prep - svec - msm
        # the object path over the first m proofs
        m = min(count, OBJ_MAX)
        shim = BatchInnerProductProver.__new__(BatchInnerProductProver)
        shim.k, shim._handle = k, None

        def objects():
            return [(u, Point.from_le64(Ps[64 * i: 64 * i + 64]), shim._proof2(i, pab, pxs, plr, trs[i], 1)) for i in range(m)]
        ready = objects()

        def object_path(items):
            bv.reset()
            for uu, PP, pr in items:
                bv.add(uu, PP, pr)
            return bv.verify()
        t_obj, _, _, v1 = median_of(lambda: object_path(ready), reps)
        t_objb, _, _, v2 = median_of(lambda: object_path(objects()), reps)
        assert v1 is True and v2 is True
        t_sub = median_of(lambda: packed(m), reps)[0]
    finally:
        bv.release()
    print("n %6d proofs %6d (%s) | packed wall %9.3f ms (min %.3f max %.3f), %.2f us a proof | device by stage events: preparation %.3f ms + s-vector sum %.3f ms + "
          "MSM %.3f ms + other %.3f ms | first %d proofs: packed %9.3f ms, object path %10.3f ms objects ready, %10.3f ms from bytes | object / packed %8.2f (ready) %8.2f (from bytes)" %
          (n, count, source, 1e3 * t_new, 1e3 * lo, 1e3 * hi, 1e6 * t_new / count, prep, svec, msm, other, m, 1e3 * t_sub, 1e3 * t_obj, 1e3 * t_objb, t_obj / t_sub, t_objb / t_sub), flush=True)
    if t_sub >= t_obj:
        print("    the packed call is NOT faster than add() + verify() with ready objects at this shape", flush=True)
    if prep > svec + msm:
        print("    the preparation kernels take more device time than the s-vector sum and the MSM together at this shape", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=400)
    ap.add_argument("--out", default="")
    ap.add_argument("--shapes", default="", help="n,proofs;n,proofs;... instead of the default list")
    ap.add_argument("--step", default="", help="internal: run one step in this process (n,proofs)")
    args = ap.parse_args()
    if args.step:
        n, count = (int(x) for x in args.step.split(","))
        step_shape(n, count, args.reps)
        return 0
    lines = ["one MI355X; every step a process of its own, one warm-up, median of %d runs; wall = host clock around a call that ends in a synchronisation; "
             "device = the engine's stage events, a run of their own" % args.reps]
    print(lines[0], flush=True)
    rc = 0
    steps = args.shapes.split(";") if args.shapes else ["%d,%d" % s for s in SHAPES]
    for step in steps:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps)], capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            lines.append("step %s: no result within %d s -- stopping" % (step, args.step_timeout))
            print(lines[-1], flush=True)
            rc = 124
            break
        out = r.stdout.rstrip("\n")
        if out:
            lines.append(out)
            print(out, flush=True)
        if r.returncode:
            lines.append("step %s: exit status %d -- stopping\n%s" % (step, r.returncode, r.stderr[-3000:]))
            print(lines[-1], flush=True)
            rc = r.returncode if r.returncode > 0 else 1
            break
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
