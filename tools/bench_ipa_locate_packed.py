#!/usr/bin/env python3
"""Naming the invalid proofs of a packed inner-product batch: the two-level plan of BatchInnerProductVerifier.locate_packed2 over
bpmi_ipa_group_values_packed_dev (group = None: default_group, then one call with group = 1) against the bisection over verify calls
(group = 0) of the same build, on the same proofs, in the same process, on one GPU:

  python tools/bench_ipa_locate_packed.py [--reps 9] [--step-timeout 900] [--out profiles/r18_ipa_locate_packed.txt]

Every step (shape) runs in a process of its own under `--step-timeout` seconds; a step that fails or runs out of time ends the run
(nothing more is started on the GPU behind it).

  shapes  (n, proofs) = (64, 2^14), (1024, 2^10); Protocol 2, every proof from the empty transcript, from the batch prover (8-bit
          tables); statements from the prover's tables in one call
  cases   0, 1 and 16 wrong statements (P_i replaced by P_(i+1), spread evenly), and one wrong statement in EVERY group of
          default_group proofs
  method  per case one warm-up of either path, then `reps` ALTERNATING calls plan / bisection; median with min and max (the spread);
          both must return the expected indices.  Wall = host clock around a call that ends in a synchronisation.  Then the plan
          alone over the valid batch, back to back
  verify  verify_packed2 over the valid batch at the start and at the end of the step: the valid-batch path of this build, to hold
          against the parent's figure for the same shape (profiles/r12_ipa_verify_packed.txt)
  device  one plan run over the valid batch (level 1 alone) and one with one wrong statement (both levels together) under the engine's
          stage events, runs of their own: preparation | half tables and grouped sum (sc_fold) | group launch and tail (msm_accumulate) |
          everything else

No threshold: the file states what was measured."""
import argparse
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [(64, 1 << 14), (1024, 1 << 10)]


def scalars(count, seed):
    """`count` packed scalars below 2^255 < q"""
    import numpy as np
    arr = np.random.default_rng(seed).integers(0, 256, size=(count, 32), dtype=np.uint8)
    arr[:, 31] &= 0x7F
    return arr.tobytes()


def spread(ts):
    return "%9.3f ms (min %.3f max %.3f)" % (1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts))


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def step_shape(n, count, reps):
    import bulletproofs_amd  # noqa: F401
    from bulletproofs_amd.ec import PackedPoints, Point, secp256k1
    from bulletproofs_amd.engine import default_engine
    from bulletproofs_amd.innerproduct import BatchInnerProductProver, BatchInnerProductVerifier
    eng = default_engine()
    k = n.bit_length() - 1
    cnt = 2 * n + 1
    raw = eng.ec_mul_batch_bytes(secp256k1.G.to_le64() * cnt, scalars(cnt, n), cnt)
    g, h = PackedPoints([None] * n, raw[: 64 * n]), PackedPoints([None] * n, raw[64 * n: 128 * n])
    u = Point.from_le64(raw[128 * n:])
    ab, bb = scalars(count * n, 7 * n + count), scalars(count * n, 11 * n + count)
    eng.set_option("prover_table_bits", 8)
    bp = BatchInnerProductProver(g, h, u, engine=eng)
    try:
        Ps = bp.commit_packed(ab, bb, "inner")
        pab, pxs, plr, trs = bp.prove2_packed(ab, bb)
    finally:
        bp.close()
        eng.set_option("prover_table_bits", 0)
    us = u.to_le64() * count
    bv = BatchInnerProductVerifier(g, h, engine=eng)
    try:
        group = bv.default_group(2, count)

        def statements(bad):
            out = bytearray(Ps)
            for i in bad:
                j = (i + 1) % count
                out[64 * i: 64 * i + 64] = Ps[64 * j: 64 * j + 64]
            return bytes(out)

        def verify_valid():
            ts = []
            assert bv.verify_packed2(us, Ps, pab, pxs, plr, trs) is True, "the batch must verify"
            for _ in range(reps):
                t, ok = timed(lambda: bv.verify_packed2(us, Ps, pab, pxs, plr, trs))
                assert ok is True
                ts.append(t)
            return ts
        print("n %5d proofs %6d default_group %4d | verify_packed2 at the start %s" % (n, count, group, spread(verify_valid())), flush=True)
        ngroups = (count + group - 1) // group
        cases = [("0 wrong", []), ("1 wrong", [count // 3]), ("16 wrong", [count // 16 * j + 5 for j in range(16)]),
                 ("every group failing (%d)" % ngroups, [group * t + (7 * t) % min(group, count - group * t) for t in range(ngroups)])]
        for name, bad in cases:
            bad = sorted(set(bad))
            Pb = statements(bad)
            plan = lambda: bv.locate_packed2(us, Pb, pab, pxs, plr, trs)
            bisect = lambda: bv.locate_packed2(us, Pb, pab, pxs, plr, trs, group=0)
            assert plan() == bad and bisect() == bad, name
            t_plan, t_bis = [], []
            for _ in range(reps):
                t, r = timed(plan)
                assert r == bad
                t_plan.append(t)
                t, r = timed(bisect)
                assert r == bad
                t_bis.append(t)
            mp, mb = statistics.median(t_plan), statistics.median(t_bis)
            print("    %-28s two-level plan %s | bisection %s | bisection / plan %7.2f%s" %
                  (name, spread(t_plan), spread(t_bis), mb / mp, "" if mp <= mb else "   <- the two-level plan LOSES here"), flush=True)
        # the valid batch again, NOT alternating: the plan's one call back to back (beside the alternating figure above, this says what the
        # bisection's idle gaps and gathers between two plan calls cost the plan's own call)
        ts = []
        for _ in range(reps + 1):
            t, r = timed(lambda: bv.locate_packed2(us, Ps, pab, pxs, plr, trs))
            assert r == []
            ts.append(t)
        print("    0 wrong, plan alone, back to back %s" % spread(ts[1:]), flush=True)
        for label, Pb in (("0 wrong, level 1 alone", Ps), ("1 wrong, levels 1 + 2", statements([count // 3]))):
            eng.profile(True)
            eng.profile_reset()
            bv.locate_packed2(us, Pb, pab, pxs, plr, trs)
            prof = eng.profile_read()
            eng.profile(False)
            prep, svec, acc = prof["rp_prepare"][0], prof["sc_fold"][0], prof["msm_accumulate"][0]
            other = sum(ms for _, (ms, _) in prof.items()) - prep - svec - acc
            print("    device by stage events, %s: preparation %.3f ms | half tables + grouped sum %.3f ms | group launch + tail %.3f ms | other %.3f ms" %
                  (label, prep, svec, acc, other), flush=True)
        print("    verify_packed2 at the end   %s" % spread(verify_valid()), flush=True)
    finally:
        bv.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--out", default="")
    ap.add_argument("--shapes", default="", help="n,proofs;n,proofs;... instead of the default list")
    ap.add_argument("--step", default="", help="internal: run one step in this process (n,proofs)")
    args = ap.parse_args()
    if args.step:
        n, count = (int(x) for x in args.step.split(","))
        step_shape(n, count, args.reps)
        return 0
    lines = ["one MI355X; every shape a process of its own; per case one warm-up of either path, then %d alternating calls plan / bisection: median (min max); "
             "wall = host clock around a call that ends in a synchronisation; device = the engine's stage events, a run of their own" % args.reps]
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
