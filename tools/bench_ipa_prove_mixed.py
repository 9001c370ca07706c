#!/usr/bin/env python3
"""One mixed call of the batched inner-product prover (MixedBatchInnerProductProver.prove2_classes_packed, bpmi_ipa_prove_batch_mixed)
against the loop of one BatchInnerProductProver per length, Protocol 2, on blocks of lengths 64 / 128 / 256 / 512 / 1 024.

    python tools/bench_ipa_prove_mixed.py [proofs per class, comma separated ...]

Default blocks: 2048,1024,512,256,256 (a service block), 64 per class, 4 per class.  Three set-ups in ONE process:
  mixed   one prover over the 1 024 generators, one table (the capacity's window width), one call per block;
  loop_a  five provers over the prefixes at the SAME window width as the shared table: isolates the launch structure;
  loop_b  five provers at each length's default width (rpp_default_table_bits): what a user ran before the mixed call.
Per block: a warm-up of each, a check that all three write the same bytes, then 9 rounds that run the three alternately; printed are
the median and range of the wall time (host clock around the call: it ends in a synchronise) and of the device time (last_ms()["total"],
summed over the loop's calls).  Table bytes and build times of the set-ups come first.  IPM_TW: window bits of the shared table (0: the
default of 1 024 elements).  IPM_LANES: engine option prover_job_lanes for every set-up (0: the rule by the launch's jobs; 16 or 64).
One JSON line per result."""
import hashlib
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bulletproofs_amd  # noqa: F401,E402
from bulletproofs_amd.engine import default_engine  # noqa: E402
from bulletproofs_amd.ec import Point, secp256k1  # noqa: E402
from bulletproofs_amd.innerproduct import BatchInnerProductProver, MixedBatchInnerProductProver  # noqa: E402

Q = secp256k1.q
NS = (64, 128, 256, 512, 1024)
N = NS[-1]
ROUNDS = 9
eng = default_engine()


def table_bytes(nbases, w):
    return nbases * ((256 + w - 1) // w) * (1 << (w - 1)) * 64


def default_bits(n):
    """rpp_default_table_bits: 16 up to 128 elements; above, the widest whose range-prover table (3 + 2n bases) stays within that of 128 at 16"""
    return 16 if n <= 128 else max(b for b in range(4, 17) if table_bytes(3 + 2 * n, b) <= table_bytes(3 + 2 * 128, 16))


def points(count):
    ks = b"".join((int.from_bytes(hashlib.sha256(b"ipm/%d" % i).digest(), "big") % Q).to_bytes(32, "little") for i in range(count))
    out = eng.ec_mul_batch_bytes(secp256k1.G.to_le64() * count, ks, count)
    return [Point.from_le64(out[64 * i: 64 * i + 64]) for i in range(count)]


def timed(make):
    eng.sync()
    t = time.perf_counter()
    obj = make()
    eng.sync()
    return obj, (time.perf_counter() - t) * 1e3


def with_bits(bits, make):
    eng.set_option("prover_table_bits", bits)
    try:
        return timed(make)
    finally:
        eng.set_option("prover_table_bits", 0)


pts = points(2 * N + 1)
g, h, u = pts[:N], pts[N: 2 * N], pts[2 * N]
TW = int(os.environ.get("IPM_TW", "0")) or default_bits(N)
LANES = int(os.environ.get("IPM_LANES", "0"))
eng.set_option("prover_job_lanes", LANES)
mixed, ms_mixed = with_bits(TW, lambda: MixedBatchInnerProductProver(g, h, u))
loop_a, loop_b, ms_a, ms_b = {}, {}, 0.0, 0.0
for n in NS:
    loop_a[n], dt = with_bits(TW, lambda: BatchInnerProductProver(g[:n], h[:n], u))
    ms_a += dt
    loop_b[n], dt = with_bits(0, lambda: BatchInnerProductProver(g[:n], h[:n], u))
    ms_b += dt
print(json.dumps({"setups": {
    "job_lanes": LANES, "mixed": {"window_bits": TW, "table_GB": round(table_bytes(2 * N + 1, TW) / 1e9, 2), "build_ms": round(ms_mixed, 1)},
    "loop_a": {"window_bits": TW, "table_GB": round(sum(table_bytes(2 * n + 1, TW) for n in NS) / 1e9, 2), "build_ms": round(ms_a, 1)},
    "loop_b": {"window_bits": [default_bits(n) for n in NS], "table_GB": round(sum(table_bytes(2 * n + 1, default_bits(n)) for n in NS) / 1e9, 2),
               "build_ms": round(ms_b, 1)}}}), flush=True)


def inputs(n, count, tag):
    def vec(name):
        return b"".join((int.from_bytes(hashlib.sha256(b"%s%d/%d/%d" % (name, tag, n, i)).digest(), "big") % Q).to_bytes(32, "little") for i in range(count * n))
    return vec(b"a"), vec(b"b")


def run_mixed(classes):
    t = time.perf_counter()
    out = mixed.prove2_classes_packed([(n, a, b, None) for n, a, b in classes])
    wall = (time.perf_counter() - t) * 1e3
    return wall, mixed.last_ms()["total"], out


def run_loop(provers, classes):
    t = time.perf_counter()
    out, dev = [], 0.0
    for n, a, b in classes:
        out.append(provers[n].prove2_packed(a, b))
        dev += provers[n].last_ms()["total"]            # (read inside the window: the loop's user would not, and it costs microseconds)
    return (time.perf_counter() - t) * 1e3, dev, out


def summary(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


blocks = [[int(x) for x in a.split(",")] for a in sys.argv[1:]] or [[2048, 1024, 512, 256, 256], [64] * 5, [4] * 5]
for tag, counts in enumerate(blocks):
    assert len(counts) == len(NS)
    classes = [(n,) + inputs(n, c, tag) for n, c in zip(NS, counts)]
    runs = {"mixed": lambda: run_mixed(classes), "loop_a": lambda: run_loop(loop_a, classes), "loop_b": lambda: run_loop(loop_b, classes)}
    warm = {name: fn() for name, fn in runs.items()}
    same = warm["mixed"][2] == warm["loop_a"][2] == warm["loop_b"][2]
    wall, dev = {name: [] for name in runs}, {name: [] for name in runs}
    for _ in range(ROUNDS):
        for name, fn in runs.items():
            w, d, _ = fn()
            wall[name].append(w)
            dev[name].append(d)
    line = {"proofs_per_class": counts, "proofs": sum(counts), "same_bytes": same, "rounds": ROUNDS}
    for name in runs:
        line[name] = {"wall_ms": summary(wall[name]), "device_ms": summary(dev[name])}
    for base in ("loop_a", "loop_b"):
        line["mixed_over_" + base] = {"wall": round(statistics.median(wall["mixed"]) / statistics.median(wall[base]), 3),
                                      "device": round(statistics.median(dev["mixed"]) / statistics.median(dev[base]), 3)}
    print(json.dumps(line), flush=True)
mixed.close()
for p in list(loop_a.values()) + list(loop_b.values()):
    p.close()
eng.set_option("prover_job_lanes", 0)
