#!/usr/bin/env python3
"""Bulk hash to the curve (bpmi_ec_hash_range_dev) on one MI355X: n generators str(i) || seed derived into device memory, for
n = 2^10, 2^16 and 2^21 -- wall time of the call (host clock; the call ends in a stream synchronise) and device time of its kernel
(the engine's stage timer: HIP events around the launch) -- and beside them
  (a) the host loop of bulletproofs_amd.utils.elliptic_hash over 2^10 messages on the same box,
  (b) bpmi_ec_decompress_batch_dev of 2n points: one square root per point, the natural ceiling for a mean of two candidates a message,
  (c) the plain one-message-per-lane loop (option h2c_plain) against the per-wave queue, run alternately, and the queue at forced
      span lengths (option h2c_per_lane).
The points of every variant are compared with each other, and the first 2^10 with the host function, before anything is timed.

    python tools/bench_hash_to_curve.py [--out FILE] [--sizes 10,16,21] [--reps 7]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SEED = b"gs"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="10,16,21")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()

    import numpy as np
    import bulletproofs_amd  # noqa: F401
    from bulletproofs_amd.engine import Engine
    from bulletproofs_amd.utils import elliptic_hash

    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    eng = Engine(device=0)
    sizes = [1 << int(e) for e in args.sizes.split(",")]
    nmax = max(sizes)
    d_out = eng.alloc(64 * 2 * nmax)

    def options(plain, per_lane):
        eng.set_option("h2c_plain", plain)
        eng.set_option("h2c_per_lane", per_lane)

    def timed(call, stage):
        """(wall ms, device ms) of one call"""
        eng.profile_reset()
        t0 = time.perf_counter()
        call()
        wall = (time.perf_counter() - t0) * 1e3
        return wall, eng.profile_read()[stage][0]

    def series(calls, stage, reps):
        """the calls run alternately, reps times each after two warm-up rounds -> [(median wall, min wall, median device, min device)]"""
        res = [[] for _ in calls]
        for r in range(reps + 2):
            for k, call in enumerate(calls):
                t = timed(call, stage)
                if r >= 2:
                    res[k].append(t)
        return [(statistics.median(w for w, _ in rs), min(w for w, _ in rs), statistics.median(d for _, d in rs), min(d for _, d in rs)) for rs in res]

    say("# bulk hash to the curve, range form str(i) || %r, points left in device memory; one MI355X" % SEED)
    say("# wall = host clock around the synchronous call, device = HIP events around the kernel; median (min) of %d runs after 2 warm-ups, variants alternated" % args.reps)
    say("# clocks as the box gives them (not locked); times in ms")

    # (a) the host loop
    t0 = time.perf_counter()
    host = b"".join(elliptic_hash(b"%d" % i + SEED).to_le64() for i in range(1024))
    host_ms = (time.perf_counter() - t0) * 1e3
    say()
    say("(a) host loop, bulletproofs_amd.utils.elliptic_hash over 2^10 messages: %.1f ms, %.3f ms per point" % (host_ms, host_ms / 1024))

    eng.profile(True)
    for n in sizes:
        e = n.bit_length() - 1
        reps = args.reps if n <= (1 << 16) else max(3, args.reps // 2 + 1)
        # correctness of what is timed: every variant gives the same points, and they are the host function's
        options(0, 0)
        eng.ec_hash_range_dev(SEED, 0, n, d_out=d_out)
        ref = d_out.download(64 * n)
        assert ref[:64 * min(n, 1024)] == host[:64 * min(n, 1024)], "device points differ from the host function's"
        variants = [("queue, span by size", 0, 0), ("plain loop", 1, 0)] + [("queue, %2d per lane" % k, 0, k) for k in (1, 2, 4, 8, 16, 32) if 64 * k <= n]
        for name, plain, per_lane in variants[1:]:
            options(plain, per_lane)
            eng.ec_hash_range_dev(SEED, 0, n, d_out=d_out)
            assert d_out.download(64 * n) == ref, name

        def hash_call(plain, per_lane):
            def call():
                options(plain, per_lane)
                eng.ec_hash_range_dev(SEED, 0, n, d_out=d_out)
            return call
        res = series([hash_call(p, k) for _, p, k in variants], "misc", reps)
        say()
        say("n = 2^%d (%d messages, %d runs each)" % (e, n, reps))
        say("  %-24s %12s %12s %14s %12s %14s" % ("(c) variant", "wall median", "wall min", "device median", "device min", "ns per point"))
        for (name, _, _), (wm, wn, dm, dn) in zip(variants, res):
            say("  %-24s %12.3f %12.3f %14.3f %12.3f %14.1f" % (name, wm, wn, dm, dn, dm * 1e6 / n))
        options(0, 0)

        # (b) decompression of 2n points: the hashed points themselves, twice, as SEC1 bytes
        arr = np.frombuffer(ref, dtype=np.uint8).reshape(n, 64)
        comp = np.concatenate([(2 + (arr[:, 32] & 1))[:, None], arr[:, 31::-1]], axis=1).astype(np.uint8)
        comp = np.concatenate([comp, comp], axis=0).tobytes()
        ok = ctypes.create_string_buffer(2 * n)

        def decompress():
            eng._ck(eng.lib.bpmi_ec_decompress_batch_dev(eng.ctx, comp, 2 * n, d_out.ptr, ok))
        decompress()
        assert ok.raw == b"\x01" * (2 * n) and d_out.download(64 * n) == ref
        (wm, wn, dm, dn), = series([decompress], "ec_decompress", reps)
        say("  %-24s %12.3f %12.3f %14.3f %12.3f %14.1f   (per root)" % ("(b) decompress 2n points", wm, wn, dm, dn, dm * 1e6 / (2 * n)))
        say("      (its wall time includes the upload of %d bytes of compressed points; the hash uploads %d)" % (len(comp), len(SEED)))

    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
