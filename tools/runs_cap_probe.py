#!/usr/bin/env python3
"""The accumulation by runs next to its cap: uniform scalars at n = 2^logn in which R scalar values are repeated K times each, so that R x 16
buckets hold K entries more than the others -- K chosen to leave the longest run just under the cap of the rule (msm_runs_cap: 128 at 2^20,
96 at 2^19), at half of it, and just over it (the device then falls back to the chunked accumulation).  Option accum_runs 0 / 1 alternating
in one process, synchronous and two in flight; results compared.   python tools/runs_cap_probe.py [logn ...]"""
import hashlib, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bulletproofs_amd  # noqa: F401
from bulletproofs_amd.engine import default_engine
from bulletproofs_amd.ec import secp256k1
Q = secp256k1.q
eng = default_engine()
logs = [int(a) for a in sys.argv[1:]] or [20, 19]


def sha_scalars(n, seed):
    pre = b"bpmi/scalar" + seed.to_bytes(8, "little")
    return [(int.from_bytes(hashlib.sha256(pre + i.to_bytes(8, "little")).digest(), "big") % Q).to_bytes(32, "little") for i in range(n)]


nmax = 1 << max(logs)
d_k = eng.upload(b"".join(sha_scalars(nmax, 1))); d_G = eng.upload(secp256k1.G.to_le64() * nmax); d_p = eng.alloc(64 * nmax)
eng._ck(eng.lib.bpmi_ec_mul_batch_dev(eng.ctx, d_G.ptr, d_k.ptr, nmax, d_p.ptr)); eng.sync()
base = sha_scalars(nmax, 2)
for lg in logs:
    n = 1 << lg
    mean = n * 16 >> 19
    cap = 2 * mean + 64
    longest_uniform = mean + 6 * int(mean ** 0.5)          # (a bound on the longest run of uniform digits, for the choice of K only)
    for R, K in ((0, 0), (1, cap - longest_uniform), (64, cap - longest_uniform), (1024, cap // 2 - mean // 2), (1, cap + 8)):
        sc = list(base[:n])
        for r in range(R):
            for k in range(K):
                sc[(r * 4099 + k * 8191 + 17) % n] = base[r]
        d_s = eng.upload(b"".join(sc))
        ref = None
        for rnd in range(3):
            for v in (0, 1):
                eng.set_option("accum_runs", v)
                r0 = eng.msm_dev(d_p, d_s, n)
                ref = ref or r0
                assert r0 == ref
                st = eng.msm_runs_state()
                t = time.perf_counter()
                for _ in range(40): eng.msm_dev(d_p, d_s, n)
                ds = (time.perf_counter() - t) / 40
                eng.set_option("async_lanes", 1)
                eng.msm_dev_enqueue(0, d_p, d_s, n)
                t = time.perf_counter()
                for j in range(40):
                    if j + 1 < 40: eng.msm_dev_enqueue((j + 1) & 1, d_p, d_s, n)
                    eng.msm_finish(j & 1)
                dp = (time.perf_counter() - t) / 40
                eng.set_option("async_lanes", 0)
                print("n=2^%d cap %d: %4d values x %3d copies  accum_runs=%d (fell back: %d)  sync %.4f ms  two in flight %.4f ms" % (lg, cap, R, K, v, st["long_run"], ds * 1e3, dp * 1e3), flush=True)
        d_s.free()
eng.set_option("accum_runs", 1)
