#!/usr/bin/env python3
"""The batched inner-product prover (innerproduct/batch_prover.py, bpmi_ipa_prove_batch) against the loop of FastNIProver2.prove over
the same inputs on the same build, and its rounds against the rounds of the batched range prover, on one GPU:

  python tools/bench_ipa_prove_batch.py [--reps 5] [--step-timeout 240] [--out profiles/r11_ipa_prove_batch.txt]

Every step runs in a process of its own under `--step-timeout` seconds; a step that fails or runs out of time ends the run (nothing
more is started on the GPU behind it).  Within a step: the generators and vectors are made once (random scalars below 2^255,
generators k_i G), ONE warm-up call of everything that is timed, then the median of `reps` runs.

  shape steps  (n, proofs) = (64, 2^14), (256, 2^12), (1024, 2^10), (64, 16), (64, 1), Protocol 2, the prover's default tables:
      batch wall     one prove2_packed call, inputs as packed bytes, host clock (the call ends in a synchronisation)
      batch device   the same call's device time (bpmi_ipa_batch_prover_last_ms: begin + head | rounds | copy out | whole)
      loop wall      FastNIProver2(...).prove() per proof over the same generators and vectors (packed once: no per-proof conversion),
                     over the first min(proofs, 256) proofs and scaled to the batch's count -- the line says so
  rounds step  2^14 proofs of 64 elements, both provers at the same table bits, measured alternately in one process:
      last_ms[rounds] of the inner-product prover against phase 3 (the rounds) of bpmi_rp_prover_last_ms: the job lists of a round
      are the same, 2 x proofs jobs of n + 1 terms

No threshold: the file states what was measured."""
import argparse
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [(64, 1 << 14), (256, 1 << 12), (1024, 1 << 10), (64, 16), (64, 1)]
LOOP_MAX = 256


def scalars(count, seed):
    """`count` packed scalars below 2^255 < q"""
    import numpy as np
    arr = np.random.default_rng(seed).integers(0, 256, size=(count, 32), dtype=np.uint8)
    arr[:, 31] &= 0x7F
    return arr.tobytes()


def setup(n, extra=0):
    import bulletproofs_amd  # noqa: F401
    from bulletproofs_amd.ec import PackedPoints, Point, secp256k1
    from bulletproofs_amd.engine import default_engine
    eng = default_engine()
    cnt = 2 * n + 1 + extra
    raw = eng.ec_mul_batch_bytes(secp256k1.G.to_le64() * cnt, scalars(cnt, n), cnt)
    g, h = PackedPoints([None] * n, raw[: 64 * n]), PackedPoints([None] * n, raw[64 * n: 128 * n])       # the wire form is all that is read
    rest = [Point.from_le64(raw[o: o + 64]) for o in range(128 * n, 64 * cnt, 64)]
    return eng, g, h, rest


def step_shape(n, count, reps):
    from bulletproofs_amd.ec import PackedScalars, secp256k1
    from bulletproofs_amd.innerproduct import BatchInnerProductProver, FastNIProver2
    eng, g, h, (u,) = setup(n)
    ab, bb = scalars(count * n, 7 * n + count), scalars(count * n, 11 * n + count)
    t0 = time.perf_counter()
    bp = BatchInnerProductProver(g, h, u, engine=eng)
    eng.sync()
    t_create = time.perf_counter() - t0
    try:
        dev = []

        def batch():
            t0 = time.perf_counter()
            out = bp.prove2_packed(ab, bb)
            dt = time.perf_counter() - t0
            dev.append(bp.last_ms())
            return dt, out
        first = batch()[1]
        walls = []
        del dev[:]
        for _ in range(reps):
            dt, out = batch()
            walls.append(dt)
            assert out == first
        mid = sorted(range(reps), key=lambda i: walls[i])[reps // 2]
        d = dev[mid]
    finally:
        bp.close()
    m = min(count, LOOP_MAX)
    rows = [(PackedScalars.from_bytes(ab[32 * n * i: 32 * n * (i + 1)]), PackedScalars.from_bytes(bb[32 * n * i: 32 * n * (i + 1)])) for i in range(m)]

    def loop():
        t0 = time.perf_counter()
        ps = [FastNIProver2(g, h, u, None, a, b, secp256k1).prove() for a, b in rows]
        eng.sync()
        return time.perf_counter() - t0, ps
    ps = loop()[1]
    # the same proofs: the first and the last of the loop against the batch's
    k = n.bit_length() - 1
    for i in (0, m - 1):
        assert ps[i].transcript == first[3][i] and ps[i].a.x.to_bytes(32, "little") == first[0][64 * i: 64 * i + 32]
        assert b"".join(pt.to_le64() for pt in ps[i].Ls + ps[i].Rs) == first[2][128 * k * i: 128 * k * (i + 1)]
    t_loop = statistics.median([loop()[0] for _ in range(reps)])
    scaled = t_loop * count / m
    wall = walls[mid]
    print("n %5d proofs %6d | batch wall %9.3f ms (min %.3f max %.3f) device %9.3f ms = begin+head %.3f + rounds %.3f + copy out %.3f | "
          "loop wall %10.3f ms%s | loop / batch %7.2f | %.2f us a proof in the batch, %.1f us in the loop | tables %d bits, built in %.0f ms" %
          (n, count, 1e3 * wall, 1e3 * min(walls), 1e3 * max(walls), d["total"], d["begin_head"], d["rounds"], d["copy_out"], 1e3 * scaled,
           " (measured over %d proofs: %.3f ms, scaled x %d)" % (m, 1e3 * t_loop, count // m) if m < count else " (measured over all)",
           scaled / wall, 1e6 * wall / count, 1e6 * scaled / count, table_bits(n), 1e3 * t_create), flush=True)
    if wall >= scaled:
        print("    the batch is NOT faster than the loop at this shape", flush=True)


def table_bits(n):
    """the default window bits (csrc/rp_prove_plan_host.hpp rpp_default_table_bits)"""
    def tb(elems, w):
        return (3 + 2 * elems) * -(-256 // w) * (1 << (w - 1)) * 64
    return 16 if n <= 128 else max(w for w in range(4, 17) if tb(n, w) <= tb(128, 16))


def step_rounds(reps):
    """2^14 proofs of 64 elements: the rounds of the inner-product prover and of the range prover, alternately."""
    from bulletproofs_amd.innerproduct import BatchInnerProductProver
    from bulletproofs_amd.rangeproofs import BatchRangeProver
    n, count = 64, 1 << 14
    eng, gs, hs, (u, g, h) = setup(n, extra=2)
    ab, bb = scalars(count * n, 1), scalars(count * n, 2)
    vb, gb = scalars(count, 3), scalars(count, 4)
    seeds = (bytes(8 * count), [8 * i for i in range(count + 1)])
    ip = BatchInnerProductProver(gs, hs, u, engine=eng)
    rp = None
    try:
        rp = BatchRangeProver(n, g, h, list(_unpacked(gs)), list(_unpacked(hs)), u, engine=eng)
        ip.prove2_packed(ab, bb)
        rp.prove_wire_packed(vb, gb, seeds, copy=False)
        pairs = []
        for _ in range(reps):
            ip.prove2_packed(ab, bb)
            a = ip.last_ms()
            rp.prove_wire_packed(vb, gb, seeds, copy=False)
            b = rp.last_ms()
            pairs.append((a["rounds"], b["ipa_rounds"], a["total"], b["total"]))
    finally:
        ip.close()
        if rp is not None:
            rp.close()
    for i, (a, b, ta, tb) in enumerate(pairs):
        print("rounds, run %d: inner-product prover %.3f ms (whole batch %.3f) | range prover phase 3 %.3f ms (whole batch %.3f) | ratio %.4f" % (i, a, ta, b, tb, a / b), flush=True)
    ma, mb = statistics.median(p[0] for p in pairs), statistics.median(p[1] for p in pairs)
    print("rounds, median of %d alternating runs, 2^14 proofs of 64 elements, %d-bit tables both: inner-product prover %.3f ms, range prover %.3f ms, ratio %.4f (%s 10 %%)" %
          (reps, table_bits(n), ma, mb, ma / mb, "within" if abs(ma / mb - 1) <= 0.10 else "NOT within"), flush=True)


def _unpacked(packed_points):
    from bulletproofs_amd.ec import Point
    raw = packed_points.packed
    return (Point.from_le64(raw[o: o + 64]) for o in range(0, len(raw), 64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default="")
    ap.add_argument("--step", default="", help="internal: run one step in this process (n,proofs or 'rounds')")
    args = ap.parse_args()
    if args.step:
        if args.step == "rounds":
            step_rounds(args.reps)
        else:
            n, count = (int(x) for x in args.step.split(","))
            step_shape(n, count, args.reps)
        return 0
    lines = ["one MI355X; every step a process of its own, one warm-up, median of %d runs; wall = host clock around a call that ends in a synchronisation" % args.reps]
    print(lines[0], flush=True)
    rc = 0
    for step in ["%d,%d" % s for s in SHAPES] + ["rounds"]:
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
