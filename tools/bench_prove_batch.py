#!/usr/bin/env python3
"""Throughput of the batched range-proof prover (bpmi_rp_prove_batch): proofs per second for a range of batch sizes, the device
milliseconds of every phase, and the one-time table build.   python tools/bench_prove_batch.py [log2 batch ...]
Environment: PB_BITS bits per value (64), PB_M values per proof (1; PB_BITS x PB_M <= 1024), PB_TW table window bits (0: the plan's
default for the size, csrc/rp_prove_plan_host.hpp), PB_OPTS engine options ("prover_job_lanes=64 ..."), PB_COMMIT=1: also
commit_packed of every batch against two batched multiplications and a batched addition."""
import hashlib, os, sys, time, json
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bulletproofs_amd  # noqa: F401
from bulletproofs_amd.engine import default_engine
from bulletproofs_amd.ec import Point, secp256k1
from bulletproofs_amd.rangeproofs import BatchRangeProver
from bulletproofs_amd.utils import ModP
Q = secp256k1.q
eng = default_engine()
nb, vm = int(os.environ.get("PB_BITS", "64")), int(os.environ.get("PB_M", "1"))
n = nb * vm                                                 # elements of a proof's vectors


def points(count, seed):
    ks = b"".join((int.from_bytes(hashlib.sha256(b"pb/%d/%d" % (seed, i)).digest(), "big") % Q).to_bytes(32, "little") for i in range(count))
    out = eng.ec_mul_batch_bytes(secp256k1.G.to_le64() * count, ks, count)
    return [Point.from_le64(out[64 * i: 64 * i + 64]) for i in range(count)]


pts = points(2 * n + 3, 1)
g, h, u, gs, hs = pts[0], pts[1], pts[2], pts[3:3 + n], pts[3 + n:]
tw = int(os.environ.get("PB_TW", "0"))
eng.set_option("prover_table_bits", tw)
for kv in os.environ.get("PB_OPTS", "").split():          # engine options, e.g. PB_OPTS="prover_split=0"
    eng.set_option(kv.split("=")[0], int(kv.split("=")[1]))
t = time.perf_counter()
bp = BatchRangeProver(nb, g, h, gs, hs, u, m=vm)
eng.sync()


def table_bytes(elems, w):
    return (3 + 2 * elems) * ((256 + w - 1) // w) * (1 << (w - 1)) * 64


# the plan's default (rpp_default_table_bits): 16 up to 128 elements, else the widest width within the table of 128 elements at 16 bits
w = tw or (16 if n <= 128 else max(b for b in range(4, 17) if table_bytes(n, b) <= table_bytes(128, 16)))
print(json.dumps({"prover_create_ms": round((time.perf_counter() - t) * 1e3, 2), "bits": nb, "values": vm, "elements": n, "table_window_bits": w,
                  "table_MB": round(table_bytes(n, w) / 1e6, 1)}), flush=True)
for lg in [int(a) for a in sys.argv[1:]] or [8, 10, 12, 14, 16]:
    m = 1 << lg
    vs = b"".join((int.from_bytes(hashlib.sha256(b"v%d" % i).digest()[:16], "big") % (1 << nb)).to_bytes(32, "little") for i in range(m * vm))
    gammas = b"".join((int.from_bytes(hashlib.sha256(b"g%d" % i).digest(), "big") % Q).to_bytes(32, "little") for i in range(m * vm))
    seeds = [b"seed-%d" % i for i in range(m)]
    bp.prove_wire_packed(vs[:32 * vm * min(m, 8)], gammas[:32 * vm * min(m, 8)], seeds[:8])
    best = None
    for rep in range(3):
        t = time.perf_counter()
        packed, off = bp.prove_wire_packed(vs, gammas, seeds)
        dt = time.perf_counter() - t
        ms = bp.last_ms()
        if best is None or dt < best[0]:
            best = (dt, ms)
    dt, ms = best
    print(json.dumps({"batch": m, "wall_ms": round(dt * 1e3, 2), "proofs_per_s_wall": round(m / dt), "proofs_per_s_device": round(m / (ms["total"] * 1e-3)),
                      "device_us_per_element": round(ms["total"] * 1e3 / (m * n), 4),
                      "device_ms": {k: round(v, 3) for k, v in ms.items()}, "bytes_per_proof": len(packed) // m}), flush=True)
    if os.environ.get("PB_COMMIT"):
        count = m * vm
        one = (1).to_bytes(32, "little")

        def three_calls():
            vg = eng.ec_mul_batch_bytes(g.to_le64() * count, vs, count)
            rh = eng.ec_mul_batch_bytes(h.to_le64() * count, gammas, count)
            return eng.ec_lincomb2_batch_bytes(vg, rh, one, one, count)
        best = {}
        for name, fn in (("commit_packed", lambda: bp.commit_packed(vs, gammas)), ("three_calls", three_calls)):
            fn()
            for rep in range(3):
                t = time.perf_counter()
                out = fn()
                best[name] = min(best.get(name, 1e9), time.perf_counter() - t)
            best[name + "_sha"] = hashlib.sha256(out).hexdigest()[:12]
        print(json.dumps({"commitments": count, "commit_packed_wall_ms": round(best["commit_packed"] * 1e3, 3), "three_calls_wall_ms": round(best["three_calls"] * 1e3, 3),
                          "same_bytes": best["commit_packed_sha"] == best["three_calls_sha"]}), flush=True)
bp.close()
