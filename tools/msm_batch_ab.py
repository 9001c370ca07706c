#!/usr/bin/env python3
"""A/B of the batched MSM (bpmi_msm_batch_dev: n_vec scalar vectors over one shared point set in one launch) against the two ways of
doing the same work one MSM at a time, on the same box, in one process, the sides alternating:
  loop      n_vec calls of bpmi_msm_dev
  rotation  bpmi_msm_dev_enqueue / bpmi_msm_finish over the three slots with "async_lanes" = 1
Seeded inputs; every shape is warmed up on every side; a side is timed with the host clock around calls that end in a device
synchronisation, repeated until a few hundred milliseconds are filled; the three sides' outputs are compared byte for byte.
  python tools/msm_batch_ab.py [--quick] [--out FILE] [--only PAIRS:ROUTE:NVEC,NVEC,... ...]
--only replaces the built-in shapes by forced-route measurements of the caller's (where a bound of the automatic plan is being placed).
Prints one line per measurement and a JSON summary; profiles/r10_msm_batch.txt is a run of it."""
import ctypes
import json
import os
import random
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bulletproofs_amd  # noqa: E402,F401
from bulletproofs_amd import _native  # noqa: E402
from bulletproofs_amd.ec import secp256k1  # noqa: E402
from bulletproofs_amd.engine import default_engine  # noqa: E402

QUICK = "--quick" in sys.argv
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
FILL_S = 0.05 if QUICK else 0.3
ROUNDS = 2 if QUICK else 3
SHAPES = [(129, 1 << 14), (2049, 1024), (8193, 64), (33792, 16), (1 << 17, 8)]          # pairs per vector x vectors
SWEEP_TOTALS = [(129, 1), (8193, 2)]                                                   # (pairs, forced route) of the min_vecs sweep
SWEEP_VECS = [1, 2, 4, 8, 16, 32, 64]
SPREAD_SHAPE = (8193, 64)
ONLY = []
if "--only" in sys.argv:
    for spec in sys.argv[sys.argv.index("--only") + 1:]:
        if spec.startswith("--"):
            break
        pairs, route, vecs = spec.split(":")
        ONLY += [(int(pairs), int(route), int(v)) for v in vecs.split(",")]
    SHAPES, SWEEP_TOTALS, SPREAD_SHAPE = [(t, v) for t, _, v in ONLY], [], None
if QUICK:
    SHAPES = [(129, 64), (2049, 16), (33793, 2)]
    SWEEP_VECS = [1, 4]
    SPREAD_SHAPE = (2049, 16)

eng = default_engine()
# the loop sides through plain integer arguments: no per-call conversion of Python objects
raw = ctypes.CDLL(_native.LIB_PATH)
_vp, _u64, _i = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
raw.bpmi_msm_dev.argtypes = [_vp, _vp, _vp, _u64, _vp]
raw.bpmi_msm_dev_enqueue.argtypes = [_vp, _i, _vp, _vp, _u64]
raw.bpmi_msm_finish.argtypes = [_vp, _i, _vp]
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


_all = SHAPES + ([SPREAD_SHAPE] if SPREAD_SHAPE else []) + [(t, max(SWEEP_VECS)) for t, _ in SWEEP_TOTALS]
max_total = max(t for t, _ in _all)
max_cells = max(t * v for t, v in _all)
rnd = random.Random(2026)
d_k = eng.upload(rnd.randbytes(32 * max_total))
d_G = eng.upload(secp256k1.G.to_le64() * max_total)
d_p = eng.alloc(64 * max_total)
eng._ck(eng.lib.bpmi_ec_mul_batch_dev(eng.ctx, d_G.ptr, d_k.ptr, max_total, d_p.ptr))      # points k_i G, k_i seeded
eng.sync()
d_s = eng.alloc(32 * max_cells)                                                          # any 256-bit values: reduced on load
for off in range(0, 32 * max_cells, 1 << 24):
    d_s.upload(rnd.randbytes(min(1 << 24, 32 * max_cells - off)), off)


def side_batch(total, n_vec, route):
    def run():
        eng.set_option("msm_batch_route", route)
        try:
            return eng.msm_batch_dev([d_p], [total], [d_s], n_vec)
        finally:
            eng.set_option("msm_batch_route", 0)
    return run


def side_loop(total, n_vec):
    out = ctypes.create_string_buffer(64 * n_vec)
    base = ctypes.addressof(out)

    def run():
        for v in range(n_vec):
            rc = raw.bpmi_msm_dev(eng.ctx, d_p.ptr, d_s.ptr + 32 * total * v, total, base + 64 * v)
            if rc:
                eng._ck(rc)
        return out.raw
    return run


def side_rotation(total, n_vec):
    out = ctypes.create_string_buffer(64 * n_vec)
    base = ctypes.addressof(out)

    def run():
        eng.set_option("async_lanes", 1)
        try:
            for v in range(n_vec + 3):                              # three in flight: MSM v takes the slot MSM v - 3 leaves
                if v >= 3:
                    eng._ck(raw.bpmi_msm_finish(eng.ctx, (v - 3) % 3, base + 64 * (v - 3)))
                if v < n_vec:
                    eng._ck(raw.bpmi_msm_dev_enqueue(eng.ctx, v % 3, d_p.ptr, d_s.ptr + 32 * total * v, total))
        finally:
            eng.set_option("async_lanes", 0)
        return out.raw
    return run


def timed(run):
    """seconds per call: calls repeated until FILL_S is filled (every call ends synchronised)"""
    reps, t0 = 0, time.perf_counter()
    while True:
        run()
        reps += 1
        dt = time.perf_counter() - t0
        if dt >= FILL_S:
            return dt / reps


def measure(total, n_vec, route, tag):
    sides = [("batch", side_batch(total, n_vec, route)), ("loop", side_loop(total, n_vec)), ("rotation", side_rotation(total, n_vec))]
    outs = [run() for _, run in sides]                                  # warm-up of every side, and the outputs
    assert outs[0] == outs[1] == outs[2], "outputs differ at %d x %d" % (total, n_vec)
    times = {name: [] for name, _ in sides}
    for _ in range(ROUNDS):
        for name, run in sides:                                         # the sides alternate
            times[name].append(timed(run))
    best = {name: min(ts) for name, ts in times.items()}
    base = min(best["loop"], best["rotation"])
    rec = {"tag": tag, "pairs": total, "n_vec": n_vec, "route": route, "ms": {k: [round(t * 1e3, 4) for t in v] for k, v in times.items()},
           "best_ms": {k: round(v * 1e3, 4) for k, v in best.items()}, "batch_over_best_baseline": round(best["batch"] / base, 4)}
    say("%-8s pairs %6d x %5d vectors route %d: batch %9.3f ms | loop %9.3f ms | rotation %9.3f ms | batch / faster baseline %.3f   (all rounds, ms: %s)"
        % (tag, total, n_vec, route, best["batch"] * 1e3, best["loop"] * 1e3, best["rotation"] * 1e3, best["batch"] / base, rec["ms"]))
    return rec


records = []
for total, route, n_vec in ONLY:
    records.append(measure(total, n_vec, route, "only"))
for total, n_vec in ([] if ONLY else SHAPES):
    records.append(measure(total, n_vec, 0, "shape"))
for total, route in SWEEP_TOTALS:
    for n_vec in SWEEP_VECS:
        records.append(measure(total, n_vec, route, "min_vecs"))
spread = [measure(SPREAD_SHAPE[0], SPREAD_SHAPE[1], 0, "spread") for _ in range(3)] if SPREAD_SHAPE else []
records += spread
for side in ("batch", "loop", "rotation") if spread else ():
    vals = [r["best_ms"][side] for r in spread]
    say("spread of %s at %d x %d over three repeats: %.4f .. %.4f ms (%.1f %%)" % (side, SPREAD_SHAPE[0], SPREAD_SHAPE[1], min(vals), max(vals),
                                                                                 100.0 * (max(vals) - min(vals)) / min(vals)))
say(json.dumps({"records": records}))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
