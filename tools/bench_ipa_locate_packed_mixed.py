#!/usr/bin/env python3
"""Naming the invalid proofs of a list of packed inner-product classes of DIFFERENT lengths: the two-level plan of
MixedBatchInnerProductVerifier.locate_packed2 over bpmi_ipa_group_values_packed_mixed_dev (group = None: default_groups, then one call
with group 1) against the bisection over mixed verify calls (group = 0) and against one single-class locate_packed2(group = None) per
length, on the same build, the same proofs, in the same process, on one GPU:

  python tools/bench_ipa_locate_packed_mixed.py [--reps 9] [--step-timeout 600] [--out profiles/r19_ipa_locate_packed_mixed.txt]

Every step (shape) runs in a process of its own under `--step-timeout` seconds; a step that fails or runs out of time ends the run
(nothing more is started on the GPU behind it).

  shapes  service: 2^12 x 64 + 2^10 x 256 + 256 x 1 024 + 16 x 2^16 (its longest class takes the msm_run route under the sqrt(count) rule);
          service-short: the same without the 2^16 class; sixteen: 4 proofs each of 64, 256, 1 024 and 4 096 elements.  Protocol 2,
          every proof from the empty transcript; `distinct` proofs per length, cycled
  cases   0, 1 and 16 wrong statements (P_i replaced by the P of another proof, spread evenly over the global index), and one wrong
          statement in every class
  method  per case one warm-up of every path, then `reps` ALTERNATING calls (a) plan / (b) bisection / (c) per-length plans; median with
          min and max; all must return the expected indices.  Wall = host clock around a call that ends in a synchronisation.  For the
          valid batch also verify_packed2
  device  one plan run over the valid batch (level 1 alone) and one with one wrong statement (both levels) under the engine's stage
          events, runs of their own: preparation | half tables and grouped sum (sc_fold) | group launches, tail and msm_run (msm_*) |
          everything else

No threshold: the file states what was measured."""
import argparse
import os
import statistics
import subprocess
import sys
import threading
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = {
    "service": [(1 << 12, 6), (1 << 10, 8), (256, 10), (16, 16)],
    "service-short": [(1 << 12, 6), (1 << 10, 8), (256, 10)],
    "sixteen": [(4, 6), (4, 8), (4, 10), (4, 12)],
}


def spread(ts):
    return "%9.3f ms (min %.3f max %.3f)" % (1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts))


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def step_shape(name, reps, distinct):
    import numpy as np
    import bulletproofs_amd  # noqa: F401
    from bulletproofs_amd.ec import PackedPoints, Point, secp256k1
    from bulletproofs_amd.engine import default_engine
    from bulletproofs_amd.innerproduct import BatchInnerProductVerifier, MixedBatchInnerProductVerifier
    from bulletproofs_amd.innerproduct._rounds import run_rounds
    from bulletproofs_amd.utils import elliptic_hash
    from bulletproofs_amd.utils.transcript import Transcript
    eng = default_engine()
    Q = secp256k1.q
    shape = SHAPES[name]

    def scalars(count, seed):                       # `count` packed scalars below 2^255 < q
        arr = np.random.default_rng(seed).integers(0, 256, size=(count, 32), dtype=np.uint8)
        arr[:, 31] &= 0x7F
        return arr.tobytes()

    K = max(k for _, k in shape)
    N = 1 << K
    raw = eng.ec_mul_batch_bytes(secp256k1.G.to_le64() * (2 * N), scalars(2 * N, K), 2 * N)
    gb, hb = raw[: 64 * N], raw[64 * N:]
    le32 = lambda v: (int(getattr(v, "x", v)) % Q).to_bytes(32, "little")

    def rows_of(k):
        """`distinct` proofs over the prefix of 2^k generators as packed rows (u, P, ab, xs, lr, transcript)"""
        n, rows = 1 << k, []
        for j in range(distinct):
            u = elliptic_hash(b"u%d-%d" % (k, j))
            ab, bb = scalars(n, 1000 * k + 2 * j), scalars(n, 1000 * k + 2 * j + 1)
            c = int.from_bytes(eng.sc_dot_bytes(ab, bb, n), "little")
            Pt = Point.from_le64(eng.msm_bytes(gb[: 64 * n] + hb[: 64 * n], ab + bb, 2 * n)) + c * u
            st, tr, xs, Ls, Rs = eng.ipa_create(gb[: 64 * n], hb[: 64 * n], ab, bb, n, u.to_le64()), Transcript(), [], [], []
            run_rounds(st, tr, Q, xs, Ls, Rs)
            a, b = st.finish()
            st.close()
            rows.append((u.to_le64(), Pt.to_le64(), le32(a) + le32(b), b"".join(le32(x) for x in xs), b"".join(p.to_le64() for p in Ls + Rs), bytes(tr.digest)))
        return rows

    made = {k: rows_of(k) for _, k in shape}
    counts = [count for count, _ in shape]
    gbase = [sum(counts[:c]) for c in range(len(shape))]
    total = sum(counts)

    def classes_with(bad):
        """The argument tuples of verify_packed2, the statements of the global indices `bad` replaced by another proof's"""
        bad, out = set(bad), []
        for c, (count, k) in enumerate(shape):
            rows = made[k]
            pick = [rows[i % distinct] for i in range(count)]
            Ps = [rows[(i + 1) % distinct][1] if gbase[c] + i in bad else r[1] for i, r in enumerate(pick)]
            out.append((b"".join(r[0] for r in pick), b"".join(Ps), b"".join(r[2] for r in pick), b"".join(r[3] for r in pick), b"".join(r[4] for r in pick), [r[5] for r in pick]))
        return out

    bv = MixedBatchInnerProductVerifier(PackedPoints([None] * N, gb), PackedPoints([None] * N, hb), engine=eng)
    singles = [BatchInnerProductVerifier(PackedPoints([None] * (1 << k), gb[: 64 << k]), PackedPoints([None] * (1 << k), hb[: 64 << k]), engine=eng) for _, k in shape]
    try:
        groups = bv.default_groups(2, [(k, None, None, count) for count, k in shape])
        print("%s: %s | default_groups %s | per-length default_group %s" % (name, " + ".join("%d x %d" % (count, 1 << k) for count, k in shape), groups,
                                                                         [sv.default_group(2, count) for sv, (count, _) in zip(singles, shape)]), flush=True)
        valid = classes_with([])
        ts = []
        assert bv.verify_packed2(valid) is True, "the batch must verify"
        for _ in range(reps):
            t, ok = timed(lambda: bv.verify_packed2(valid))
            assert ok is True
            ts.append(t)
        print("    verify_packed2 over the valid batch %s" % spread(ts), flush=True)
        cases = [("0 wrong", []), ("1 wrong", [total // 3]), ("16 wrong", sorted({(total * j) // 16 + 1 for j in range(16)}) if total > 16 else list(range(total))),
                 ("one wrong in every class (%d)" % len(shape), [gbase[c] + counts[c] // 2 for c in range(len(shape))])]
        for label, bad in cases:
            bad = sorted(set(bad))
            cls = classes_with(bad)
            plan = lambda: bv.locate_packed2(cls, group=None)
            bisect = lambda: bv.locate_packed2(cls, group=0)
            per_length = lambda: sorted(gbase[c] + i for c, (sv, cl) in enumerate(zip(singles, cls)) for i in sv.locate_packed2(*cl, group=None))
            paths = (plan, bisect, per_length)
            for f in paths:
                assert f() == bad, label
            tss = ([], [], [])
            for _ in range(reps):
                for f, acc in zip(paths, tss):
                    t, r = timed(f)
                    assert r == bad
                    acc.append(t)
            ma, mb, mc = (statistics.median(x) for x in tss)
            notes = ("   <- the plan LOSES to the bisection" if ma > mb else "") + ("   <- the plan LOSES to the per-length plans" if ma > mc else "")
            print("    %-30s (a) plan %s | (b) bisection %s | (c) per length %s | b / a %6.2f  c / a %5.2f%s" % (label, spread(tss[0]), spread(tss[1]), spread(tss[2]), mb / ma, mc / ma, notes),
                  flush=True)
        for label, bad in (("0 wrong, level 1 alone", []), ("1 wrong, levels 1 + 2", [total // 3])):
            cls = classes_with(bad)
            eng.profile(True)
            eng.profile_reset()
            bv.locate_packed2(cls, group=None)
            prof = {k: v[0] for k, v in eng.profile_read().items() if v[1]}
            eng.profile(False)
            prep, svec = prof.get("rp_prepare", 0.0), prof.get("sc_fold", 0.0)
            msm = sum(ms for k, ms in prof.items() if k.startswith("msm_"))
            print("    device by stage events, %s: preparation %.3f ms | half tables + grouped sum %.3f ms | group launches, tail, msm_run %.3f ms | other %.3f ms" %
                  (label, prep, svec, msm, sum(prof.values()) - prep - svec - msm), flush=True)
    finally:
        for v in [bv] + singles:
            v.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--out", default="")
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--step", default="", help="internal: run one shape in this process")
    args = ap.parse_args()
    if args.step:
        step_shape(args.step, args.reps, args.distinct)
        return 0
    lines = ["one MI355X; every shape a process of its own; Protocol 2; per case one warm-up of every path, then %d alternating calls (a) locate_packed2(group=None) / "
             "(b) group=0, the bisection / (c) one single-class locate_packed2(group=None) per length: median (min max); wall = host clock around a call that ends in a "
             "synchronisation; device = the engine's stage events, a run of their own; %d distinct proofs per length, cycled" % (args.reps, args.distinct)]
    print(lines[0], flush=True)
    rc = 0
    for step in args.shapes:
        # the step's lines are passed on as they come (a long step is never silent); a timer ends a step that runs out of time
        proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps), "--distinct", str(args.distinct)], stdout=subprocess.PIPE,
                                stderr=subprocess.PIPE, text=True)
        late = []
        timer = threading.Timer(args.step_timeout, lambda: (late.append(1), proc.kill()))
        timer.start()
        try:
            for line in proc.stdout:
                lines.append(line.rstrip("\n"))
                print(lines[-1], flush=True)
            err = proc.stderr.read()
            proc.wait()
        finally:
            timer.cancel()
        if late:
            lines.append("step %s: no result within %d s -- stopping" % (step, args.step_timeout))
            print(lines[-1], flush=True)
            rc = 124
            break
        if proc.returncode:
            lines.append("step %s: exit status %d -- stopping\n%s" % (step, proc.returncode, err[-3000:]))
            print(lines[-1], flush=True)
            rc = proc.returncode if proc.returncode > 0 else 1
            break
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
