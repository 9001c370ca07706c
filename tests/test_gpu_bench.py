"""bench.py without --full: the headline line alone, and --dump-outputs writes the result of the last timed step, which must be the
known answer (sum e_i k_i mod q) * G of the benchmark's seeded inputs (computed here by the C oracle)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def test_plain_bench_line_and_dumped_result(tmp_path):
    from benchlib.common import Q, synth_scalars
    from oracle import cbind
    from oracle.ec import secp256k1

    logn, steps = 14, 3
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--logn", str(logn),
           "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["unit"] == "pairs/s" and out["higher_is_better"] is True and out["steps"] == steps and out["dtype"]
    assert out["ms_per_step"] > 0 and abs(out["value"] - (1 << logn) / (out["ms_per_step"] / 1e3)) <= 1e-6 * out["value"]
    assert not {"extra", "cpu_baseline", "roofline", "result_ok", "summary"} & set(out)

    got = np.load(tmp_path / "out" / "msm_result.npy")
    assert got.dtype == np.float32 and got.shape == (2, 32)
    _, kv = synth_scalars(1 << logn, 1000)
    _, ev = synth_scalars(1 << logn, 0)
    want = cbind.pack_points(cbind.ec_mul_batch([secp256k1.G], [sum(e * k for e, k in zip(ev, kv)) % Q]))
    assert bytes(got.astype(np.uint8).tobytes()) == want
