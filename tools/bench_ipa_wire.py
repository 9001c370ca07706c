#!/usr/bin/env python3
"""Inner-product proofs verified from their wire format BPIP2 (BatchInnerProductVerifier.verify_wire2, bpmi_ipa_verify_batch_wire_dev)
against the packed call of the same build (verify_packed2, bpmi_ipa_verify_batch_packed_dev) on the same proofs, in one process, on
one GPU:

  python tools/bench_ipa_wire.py [--reps 9] [--step-timeout 400] [--out profiles/r23_ipa_verify_wire.txt]
  python tools/bench_ipa_wire.py --packed-only ...      verify_packed2 alone: runs on a tree without the wire format too

Every step runs in a process of its own under `--step-timeout` seconds; a step that fails or runs out of time ends the run (nothing
more is started on the GPU behind it).  Within a step the generators, witnesses, statements (one commit call) and proofs are made
once, both calls run once as a warm-up, then `reps` calls of each ALTERNATE and the medians are reported.

  shapes  (n, proofs) = (64, 2^14), (256, 2^12), (1024, 2^10), (64, 16), (64, 1) from the batch prover (8-bit tables: the proofs do
          not depend on them), and (2^16, 64) with proofs from FastNIProver2; Protocol 2, every proof from the empty transcript
  wall    one verify call, host clock (the call ends in a synchronisation).  The packed call takes the list of transcripts the prover
          returned (it joins them), the wire call the joined blobs and their offsets as prove2_wire returns them
  device  the same call under the engine's stage events, a run of its own: decompression ("ec_decompress") | expansion (memset of T,
          expander, offsets: "rp_elements") | preparation ("rp_prepare" less the expansion, which its timer encloses) | s-vector sum
          ("sc_fold") | the MSM's stages
  upload  the bytes a call sends: the proofs, their offsets and the statements u, P

No threshold: the file states what was measured."""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [(64, 1 << 14), (256, 1 << 12), (1024, 1 << 10), (1 << 16, 64), (64, 16), (64, 1)]
Q = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


def scalars(count, seed):
    """`count` packed scalars below 2^255 < q"""
    import numpy as np
    arr = np.random.default_rng(seed).integers(0, 256, size=(count, 32), dtype=np.uint8)
    arr[:, 31] &= 0x7F
    return arr.tobytes()


def alternate(fns, reps):
    """Median, min, max of `reps` calls of each function, taken in turns after one warm-up each."""
    for fn in fns:
        assert fn() is True, "the batch must verify"
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(ts, fns):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def stages(eng, fn):
    eng.profile(True)
    eng.profile_reset()
    fn()
    prof = eng.profile_read()
    eng.profile(False)
    ms = lambda name: prof[name][0]
    msm = sum(v for name, (v, _) in prof.items() if name.startswith("msm_"))
    return {"decompression": ms("ec_decompress"), "expansion": ms("rp_elements"), "preparation": ms("rp_prepare") - ms("rp_elements"), "s-vector sum": ms("sc_fold"),
            "MSM": msm}


def step_shape(n, count, reps, packed_only):
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
    us = u.to_le64() * count
    if n <= 1024:
        eng.set_option("prover_table_bits", 8)
        bp = BatchInnerProductProver(g, h, u, engine=eng)
        try:
            Ps = bp.commit_packed(ab, bb, "inner")
            pab, pxs, plr, trs = bp.prove2_packed(ab, bb)
        finally:
            bp.close()
            eng.set_option("prover_table_bits", 0)
        source = "batch prover"
    else:
        Ps, pab, pxs, plr, trs = b"", b"", b"", b"", []
        for p in range(count):
            a_row, b_row = ab[32 * n * p: 32 * n * (p + 1)], bb[32 * n * p: 32 * n * (p + 1)]
            Ps += eng.msm_bytes(raw, a_row + b_row + eng.sc_dot_bytes(a_row, b_row, n), cnt)
            pr = FastNIProver2(g, h, u, None, PackedScalars.from_bytes(a_row), PackedScalars.from_bytes(b_row), secp256k1).prove()
            pab += (pr.a.x % Q).to_bytes(32, "little") + (pr.b.x % Q).to_bytes(32, "little")
            pxs += b"".join((x.x % Q).to_bytes(32, "little") for x in pr.xs)
            plr += b"".join(pt.to_le64() for pt in pr.Ls + pr.Rs)
            trs.append(pr.transcript)
        source = "FastNIProver2"
    bv = BatchInnerProductVerifier(g, h, engine=eng)
    try:
        packed = lambda: bv.verify_packed2(us, Ps, pab, pxs, plr, trs)
        up_packed = len(pab) + len(pxs) + len(plr) + sum(len(t) for t in trs) + 8 * (count + 1) + 128 * count
        head = "n %6d proofs %6d (%s)" % (n, count, source)
        if packed_only:
            ((t, lo, hi),) = alternate([packed], reps)
            print("%s | verify_packed2 wall %9.3f ms (min %.3f max %.3f)" % (head, 1e3 * t, 1e3 * lo, 1e3 * hi), flush=True)
            return
        from bulletproofs_amd.innerproduct.codec import wire_from_packed
        blobs, off = wire_from_packed(pab, pxs, plr, trs)
        off = (ctypes.c_uint64 * (count + 1))(*off)
        wire = lambda: bv.verify_wire2(us, Ps, blobs, off)
        up_wire = len(blobs) + 8 * (count + 1) + 128 * count
        (tp, plo, phi), (tw, wlo, whi) = alternate([packed, wire], reps)
        sp, sw = stages(eng, packed), stages(eng, wire)
    finally:
        bv.release()
    fmt = lambda s: " + ".join("%s %.3f" % (name, v) for name, v in s.items() if v > 0)
    print("%s | wire wall %9.3f ms (min %.3f max %.3f) | packed wall %9.3f ms (min %.3f max %.3f) | packed / wire %.2f | upload: wire %d B, packed %d B (%.2fx) | "
          "device ms, wire: %s = %.3f | device ms, packed: %s = %.3f" %
          (head, 1e3 * tw, 1e3 * wlo, 1e3 * whi, 1e3 * tp, 1e3 * plo, 1e3 * phi, tp / tw, up_wire, up_packed, up_packed / up_wire, fmt(sw), sum(sw.values()),
           fmt(sp), sum(sp.values())), flush=True)
    if tw >= tp:
        print("    the wire call is NOT faster than the packed call at this shape", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--step-timeout", type=int, default=400)
    ap.add_argument("--out", default="")
    ap.add_argument("--packed-only", action="store_true")
    ap.add_argument("--shapes", default="", help="n,proofs;n,proofs;... instead of the default list")
    ap.add_argument("--step", default="", help="internal: run one step in this process (n,proofs)")
    args = ap.parse_args()
    if args.step:
        n, count = (int(x) for x in args.step.split(","))
        step_shape(n, count, args.reps, args.packed_only)
        return 0
    lines = ["one MI355X; every step a process of its own, one warm-up, medians of %d alternating calls; wall = host clock around a call that ends in a "
             "synchronisation; device = the engine's stage events, a run of their own" % args.reps]
    print(lines[0], flush=True)
    rc = 0
    steps = args.shapes.split(";") if args.shapes else ["%d,%d" % s for s in SHAPES]
    for step in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps)] + (["--packed-only"] if args.packed_only else [])
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
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
