#!/usr/bin/env python3
"""The fixed-base MSM (bpmi_fixed_base_*, bpmi_msm_fixed_dev*) against bpmi_msm_dev / bpmi_msm_dev_enqueue of the same build, default
options, the same points and scalars, in one process, the two sides alternating call by call.
  python tools/bench_msm_fixed.py [--quick] [--out FILE] [--sizes LOG2,LOG2,...] [--widths C,C,...] [--rows R,R,...]
Grid: n in 2^13, 2^14, 2^16, 2^18, 2^19 and 2^20 (rows <= 8 there: n x rows <= 2^23), window bits 13 .. 16, rows 1, 2, 4, 8 and W.
Every size runs in a child process of its own under `timeout`; per (size, window bits, rows) the child reports
  one    milliseconds per MSM one at a time: the median of REPS timed calls after warm-up (host clock around a synchronous call), both sides
  pair   milliseconds per MSM with two in flight through the asynchronous pair (slots 0 / 1, "async_lanes" = 1), both sides
  build  table build in ms, and the table's bytes
  stages device time per MSM of the fixed side's stages from bpmi_profile, in a run of its own: sort (recoding, scans, partition, level B),
         accumulate, scan (segmented), reduce, tail
and, per size, the spread of the baseline's medians over the configurations of that process (the same code measured again and again):
a table wins only by more than that.  Outputs are compared byte for byte.  profiles/r14_msm_fixed.txt is a run of it."""
import ctypes
import json
import os
import random
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

QUICK = "--quick" in sys.argv


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


REPS = 8 if QUICK else 24
WARM = 2 if QUICK else 4
SIZES = [int(x) for x in _arg("--sizes", "10,12" if QUICK else "13,14,16,18,19,20").split(",")]
WIDTHS = [int(x) for x in _arg("--widths", "16" if QUICK else "13,14,15,16").split(",")]
ROWS = [x for x in _arg("--rows", "1,4,W" if QUICK else "1,2,4,8,W").split(",")]
OUT = _arg("--out", None)
STAGES = {"sort": ("msm_digits_hist", "msm_scan", "msm_scatter", "misc"), "accumulate": ("msm_accumulate",), "scan": ("msm_segscan",),
          "reduce": ("msm_bucket_reduce",), "tail": ("msm_tail",)}


def child(logn):
    import bulletproofs_amd  # noqa: F401
    from bulletproofs_amd import _native
    from bulletproofs_amd.ec import secp256k1
    from bulletproofs_amd.engine import default_engine
    eng = default_engine()
    raw = ctypes.CDLL(_native.LIB_PATH)             # plain integer arguments: no per-call conversion of Python objects
    _vp, _u64, _i = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    raw.bpmi_msm_dev.argtypes = [_vp, _vp, _vp, _u64, _vp]
    raw.bpmi_msm_dev_enqueue.argtypes = [_vp, _i, _vp, _vp, _u64]
    raw.bpmi_msm_finish.argtypes = [_vp, _i, _vp]
    raw.bpmi_msm_fixed_dev.argtypes = [_vp, _vp, _u64, _vp]
    raw.bpmi_msm_fixed_dev_enqueue.argtypes = [_vp, _i, _vp, _u64]
    n = 1 << logn
    rnd = random.Random(2026 + logn)
    d_k, d_G, d_p = eng.upload(rnd.randbytes(32 * n)), eng.upload(secp256k1.G.to_le64() * n), eng.alloc(64 * n)
    eng._ck(eng.lib.bpmi_ec_mul_batch_dev(eng.ctx, d_G.ptr, d_k.ptr, n, d_p.ptr))      # points k_i G, k_i seeded
    eng.sync()
    d_G.free()
    d_s = eng.upload(rnd.randbytes(32 * n))                                              # any 256-bit values: reduced on load
    out = ctypes.create_string_buffer(64)
    ctx = eng.ctx

    def base_one():
        eng._ck(raw.bpmi_msm_dev(ctx, d_p.ptr, d_s.ptr, n, out))

    def pair(enqueue):
        """seconds per MSM with two in flight: MSM j + 1 is queued before MSM j is finished"""
        eng.set_option("async_lanes", 1)
        try:
            count = REPS + 2
            enqueue(0)
            t0 = time.perf_counter()
            for j in range(count):
                if j + 1 < count:
                    enqueue((j + 1) & 1)
                eng._ck(raw.bpmi_msm_finish(ctx, j & 1, out))
            return (time.perf_counter() - t0) / count
        finally:
            eng.set_option("async_lanes", 0)

    def base_enqueue(slot):
        eng._ck(raw.bpmi_msm_dev_enqueue(ctx, slot, d_p.ptr, d_s.ptr, n))

    def one_time(run):
        t0 = time.perf_counter()
        run()
        return time.perf_counter() - t0

    for _ in range(WARM):
        base_one()
    want = out.raw
    records = []
    for c in WIDTHS:
        W = 255 // c + 1
        for spec in ROWS:
            rows = W if spec == "W" else int(spec)
            Wv = -(-W // rows)
            R = -(-W // Wv)
            if rows > W or n * R > 1 << 23:
                continue
            fx = eng.fixed_base_create(d_p, n, c, rows)
            info = fx.info
            h = fx.handle

            def fixed_one():
                eng._ck(raw.bpmi_msm_fixed_dev(h, d_s.ptr, n, out))

            def fixed_enqueue(slot):
                eng._ck(raw.bpmi_msm_fixed_dev_enqueue(h, slot, d_s.ptr, n))

            for _ in range(WARM):
                base_one()
                fixed_one()
            assert out.raw == want, "outputs differ at n = 2^%d, c = %d, rows = %d" % (logn, c, rows)
            tb, tf = [], []
            for _ in range(REPS):                                  # the sides alternate call by call
                tb.append(one_time(base_one))
                tf.append(one_time(fixed_one))
            pair(base_enqueue)
            pair(fixed_enqueue)
            pb = [pair(base_enqueue), pair(fixed_enqueue), pair(base_enqueue), pair(fixed_enqueue)]
            eng.profile(True)                                      # the stages, in a run of their own (the events cost time between kernels)
            eng.profile_reset()
            for _ in range(5):
                fixed_one()
            prof = eng.profile_read()
            eng.profile(False)
            stages = {k: round(1e3 * sum(prof[s][0] for s in names) / 5, 1) for k, names in STAGES.items()}
            fx.close()
            rec = {"log2n": logn, "c": c, "rows": R, "Wv": info["virtual_windows"], "table_bytes": info["table_bytes"], "build_ms": round(info["build_us"] / 1e3, 3),
                   "one_ms": {"fixed": round(1e3 * statistics.median(tf), 4), "base": round(1e3 * statistics.median(tb), 4),
                              "fixed_min": round(1e3 * min(tf), 4), "base_min": round(1e3 * min(tb), 4)},
                   "pair_ms": {"fixed": round(1e3 * min(pb[1], pb[3]), 4), "base": round(1e3 * min(pb[0], pb[2]), 4)}, "stages_us": stages}
            records.append(rec)
            print("n 2^%-2d c %2d rows %2d Wv %2d | one at a time: fixed %7.4f ms, bpmi_msm_dev %7.4f ms (%.3f) | two in flight: fixed %7.4f, baseline %7.4f (%.3f) | "
                  "table %9.1f KB built in %8.3f ms | us: %s" % (logn, c, R, rec["Wv"], rec["one_ms"]["fixed"], rec["one_ms"]["base"], rec["one_ms"]["fixed"] / rec["one_ms"]["base"],
                                                               rec["pair_ms"]["fixed"], rec["pair_ms"]["base"], rec["pair_ms"]["fixed"] / rec["pair_ms"]["base"],
                                                               info["table_bytes"] / 1024, rec["build_ms"], " ".join("%s %.0f" % kv for kv in stages.items())), flush=True)
    bases = [r["one_ms"]["base"] for r in records]
    if bases:
        print("n 2^%-2d baseline medians over %d configurations: %.4f .. %.4f ms (spread %.1f %%)" % (logn, len(bases), min(bases), max(bases),
                                                                                                  100.0 * (max(bases) - min(bases)) / min(bases)), flush=True)
    print("JSON " + json.dumps(records), flush=True)


def main():
    lines = ["$ python tools/bench_msm_fixed.py " + " ".join(a for a in sys.argv[1:] if a != "--out" and a != OUT)]
    print(lines[0], flush=True)
    records = []
    for logn in SIZES:
        limit = 120 + (60 << max(0, logn - 16))
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", str(logn)] + [a for a in sys.argv[1:] if a != "--out" and a != OUT]
        r = subprocess.run(cmd, capture_output=True, text=True)
        for line in r.stdout.splitlines():
            if line.startswith("JSON "):
                records += json.loads(line[5:])
            else:
                print(line, flush=True)
                lines.append(line)
        if r.returncode:
            # a child that failed, faulted or ran into its limit ends the run: nothing more is started on the device
            lines.append("n 2^%d: the child ended with status %d: %s" % (logn, r.returncode, r.stderr[-2000:]))
            print(lines[-1], flush=True)
            break
    best = {}
    for r in records:
        k = r["log2n"]
        if k not in best or r["one_ms"]["fixed"] < best[k]["one_ms"]["fixed"]:
            best[k] = r
    for k in sorted(best):
        r = best[k]
        lines.append("best at 2^%d: c %d rows %d: %.4f ms against %.4f ms" % (k, r["c"], r["rows"], r["one_ms"]["fixed"], r["one_ms"]["base"]))
        print(lines[-1], flush=True)
    lines.append(json.dumps({"records": records}))
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if len({r["log2n"] for r in records}) < len(SIZES) else 0


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(int(sys.argv[sys.argv.index("--child") + 1]))
    else:
        sys.exit(main())
