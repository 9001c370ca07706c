#!/usr/bin/env python3
"""The statements of a batch from the inner-product prover's tables (bpmi_ipa_batch_prover_commit_batch, BatchInnerProductProver.
commit_packed) against what the library offered for them before, bpmi_msm_batch_dev over [g | h | u], on one GPU, on the same build and
in the same process, the two alternating call by call:

  python tools/bench_ipa_commit.py [--reps 9] [--step-timeout 240] [--shapes N,COUNT ...] [--job-lanes 64] [--out profiles/r15_ipa_commit_batch.txt]

Every shape runs in a process of its own under `--step-timeout` seconds; a step that fails or runs out of time ends the run (nothing
more is started on the GPU behind it).  Within a step: generators k_i G and scalars below 2^255 made once, the prover's default
tables, ONE warm-up call of each side (outputs compared byte for byte), then `reps` alternating pairs of calls; medians, and the
baseline's spread (min .. max).

  commit wall     commit_packed(a, b, t) from host bytes to host bytes, host clock (checks, staging, both copies; ends synchronised)
  commit device   the same call's three kernels by HIP events (bpmi_ipa_batch_prover_commit_last_ms)
  msm_batch dev   bpmi_msm_batch_dev with points and scalars RESIDENT on the device, host clock around the call (it ends synchronised
                  and copies the results down): its device time plus the launches -- the figure of profiles/r10_msm_batch.txt
  msm_batch wall  the upload of the same scalars from host bytes plus that call: what a caller starting from host vectors pays
  rounds          last_ms[rounds] of bpmi_ipa_prove_batch (Protocol 2) on the same batch from the same prover, and the ratio
                  (2n + 1) / (2k(n + 1)) of a statement's terms to the rounds' that addition counts predict for commit device / rounds

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


def scalars(count, seed):
    """`count` scalars below 2^255 < q as a (count, 32) array of bytes"""
    import numpy as np
    arr = np.random.default_rng(seed).integers(0, 256, size=(count, 32), dtype=np.uint8)
    arr[:, 31] &= 0x7F
    return arr


def step_shape(n, count, reps, job_lanes=0):
    import numpy as np
    import bulletproofs_amd  # noqa: F401
    from bulletproofs_amd.ec import PackedPoints, Point, secp256k1
    from bulletproofs_amd.engine import default_engine
    from bulletproofs_amd.innerproduct import BatchInnerProductProver
    eng = default_engine()
    eng.set_option("prover_job_lanes", job_lanes)
    nb = 2 * n + 1
    raw = eng.ec_mul_batch_bytes(secp256k1.G.to_le64() * nb, scalars(nb, n).tobytes(), nb)
    g, h, u = PackedPoints([None] * n, raw[: 64 * n]), PackedPoints([None] * n, raw[64 * n: 128 * n]), Point.from_le64(raw[128 * n:])
    a, b, t = scalars(count * n, 3 * n + count), scalars(count * n, 5 * n + count), scalars(count, 7 * n + count)
    ab, bb, tb = a.tobytes(), b.tobytes(), t.tobytes()
    rows = np.concatenate([a.reshape(count, 32 * n), b.reshape(count, 32 * n), t], axis=1).tobytes()      # row p: a_p | b_p | t_p over [g | h | u]
    d_pts = eng.upload(raw)
    d_rows = eng.upload(rows)
    d_up = eng.alloc(len(rows))
    bp = BatchInnerProductProver(g, h, u, engine=eng)
    try:
        def commit():
            t0 = time.perf_counter()
            out = bp.commit_packed(ab, bb, tb)
            return time.perf_counter() - t0, bp.commit_last_ms()["device"], out

        def base_dev():
            t0 = time.perf_counter()
            out = eng.msm_batch_dev([d_pts], [nb], [d_rows], count)
            return time.perf_counter() - t0, out

        def base_wall():
            t0 = time.perf_counter()
            d_up.upload(rows)
            out = eng.msm_batch_dev([d_pts], [nb], [d_up], count)
            return time.perf_counter() - t0, out
        first = commit()[2]
        assert base_dev()[1] == first and base_wall()[1] == first, "the two sides differ"
        cw, cd, bd, bw = [], [], [], []
        for _ in range(reps):                                           # the sides alternate, call by call
            w, d, out = commit()
            cw.append(w)
            cd.append(d)
            bd.append(base_dev()[0])
            bw.append(base_wall()[0])
            assert out == first
        rounds = []
        for _ in range(3):
            bp.prove2_packed(ab, bb)
            rounds.append(bp.last_ms()["rounds"])
    finally:
        bp.close()
    med = statistics.median
    k = n.bit_length() - 1
    predicted = (2 * n + 1) / (2 * k * (n + 1))
    print("n %5d statements %6d%s | commit wall %8.3f ms (min %.3f max %.3f) device %8.3f ms (min %.3f max %.3f) | msm_batch_dev resident %8.3f ms (min %.3f max %.3f) "
          "from host bytes %8.3f ms (min %.3f max %.3f) | resident / commit device %6.2f, from host / commit wall %6.2f | rounds of prove_batch %8.3f ms, "
          "commit device / rounds %.4f, terms predict %.4f | medians of %d alternating calls" %
          (n, count, " (prover_job_lanes %d)" % job_lanes if job_lanes else "", 1e3 * med(cw), 1e3 * min(cw), 1e3 * max(cw), med(cd), min(cd), max(cd), 1e3 * med(bd), 1e3 * min(bd), 1e3 * max(bd),
           1e3 * med(bw), 1e3 * min(bw), 1e3 * max(bw), 1e3 * med(bd) / med(cd), med(bw) / med(cw), med(rounds), med(cd) / med(rounds), predicted, reps), flush=True)
    if med(cw) >= min(bw) or med(cd) >= 1e3 * min(bd):
        print("    the new call is NOT ahead of bpmi_msm_batch_dev at this shape beyond the baseline's spread", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default="")
    ap.add_argument("--shapes", nargs="*", default=[], help="n,statements ... instead of the built-in shapes (where a crossover is being placed)")
    ap.add_argument("--job-lanes", type=int, default=0, choices=[0, 16, 64], help="engine option prover_job_lanes (0: the automatic rule)")
    ap.add_argument("--step", default="", help="internal: run one shape in this process (n,statements)")
    args = ap.parse_args()
    if args.reps < 9:
        ap.error("at least 9 repetitions")
    if args.step:
        n, count = (int(x) for x in args.step.split(","))
        step_shape(n, count, args.reps, args.job_lanes)
        return 0
    lines = ["one MI355X; every shape a process of its own, one warm-up, medians of %d alternating calls; default tables; u_mode 2 (explicit t) against "
             "bpmi_msm_batch_dev over [g | h | u], outputs equal byte for byte" % args.reps]
    print(lines[0], flush=True)
    rc = 0
    for step in args.shapes or ["%d,%d" % s for s in SHAPES]:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps), "--job-lanes", str(args.job_lanes)], capture_output=True, text=True, timeout=args.step_timeout)
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
