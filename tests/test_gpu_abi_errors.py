"""Error behaviour of the C-ABI on a live GPU: negative codes + messages, never a crash;
state-machine errors of the IPA object; option validation."""
import ctypes

import pytest

from helpers import Q
from oracle import cbind

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gp():
    import gpu_common
    return gpu_common


def test_argument_errors(gp):
    from bulletproofs_amd.engine import EngineError
    eng = gp.engine()
    lib, ctx = eng.lib, eng.ctx
    out = ctypes.create_string_buffer(64)
    assert lib.bpmi_msm(ctx, None, None, 5, out) == -3
    assert b"null" in lib.bpmi_last_error(ctx)
    assert lib.bpmi_msm(ctx, b"", b"", 0, out) == 0 and out.raw == bytes(64)
    assert lib.bpmi_msm_dev(ctx, 1, 1, (1 << 26) + 1, out) == -3
    assert b"BPMI_MAX_N" in lib.bpmi_last_error(ctx)
    assert lib.bpmi_msm(None, b"", b"", 0, out) == -3
    assert lib.bpmi_set_option(ctx, b"window_bits", 17) == -3
    assert lib.bpmi_set_option(ctx, b"no_such_option", 1) == -3
    assert lib.bpmi_set_option(ctx, b"window_bits", 0) == 0
    with pytest.raises(EngineError, match="window_bits"):
        eng.set_option("window_bits", 1)
    assert lib.bpmi_ec_sum(ctx, None, 0, out) == 0 and out.raw == bytes(64)
    out32 = ctypes.create_string_buffer(32)
    assert lib.bpmi_sc_dot(ctx, None, None, 0, out32) == 0 and out32.raw == bytes(32)


def test_ipa_state_errors(gp):
    eng = gp.engine()
    pts, _ = gp.rand_points(9, 77)
    g, h, u = pts[:4], pts[4:8], pts[8]
    a, b = [3, 5, 7, 11], [13, 17, 19, 23]
    st = ctypes.c_void_p()
    # length must be a power of two
    rc = eng.lib.bpmi_ipa_create(eng.ctx, cbind.pack_points(g[:3]), cbind.pack_points(h[:3]), cbind.pack_scalars(a[:3]),
                                 cbind.pack_scalars(b[:3]), 3, cbind.pack_points([u]), ctypes.byref(st))
    assert rc == -3
    s = eng.ipa_create(cbind.pack_points(g), cbind.pack_points(h), cbind.pack_scalars(a), cbind.pack_scalars(b), 4,
                       cbind.pack_points([u]))
    A32, B32 = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    assert eng.lib.bpmi_ipa_finish(s.handle, A32, B32) == -5          # not reduced yet
    for _ in range(2):
        s.round_LR()
        s.fold(5, pow(5, -1, Q))
    L, R = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    assert eng.lib.bpmi_ipa_round_LR(s.handle, L, R) == -5           # already length 1
    assert eng.lib.bpmi_ipa_fold(s.handle, (5).to_bytes(32, "little"), (5).to_bytes(32, "little")) == -5
    fa, fb = s.finish()
    x, xi = 5, pow(5, -1, Q)
    a1 = [(x * a[0] + xi * a[2]) % Q, (x * a[1] + xi * a[3]) % Q]
    assert fa == (x * a1[0] + xi * a1[1]) % Q
    s.close()


def test_profile_interface(gp):
    eng = gp.engine()
    pts, _ = gp.rand_points(300, 3)
    pb, sb = cbind.pack_points(pts), cbind.pack_scalars(list(range(1, 301)))
    eng.profile(True)
    eng.profile_reset()
    eng.msm_bytes(pb, sb, 300)
    eng.msm_bytes(pb, sb, 300)
    prof = eng.profile_read()
    eng.profile(False)
    assert prof["msm_accumulate"][1] == 2 and prof["msm_accumulate"][0] > 0
    assert set(prof) >= {"msm_digits_hist", "msm_scatter", "msm_tail", "ec_lincomb2", "sc_dot"}


def test_c_program_through_the_abi_only(tmp_path):
    """examples/msm_c_abi.c: a C99 program that uses nothing but include/bpmi.h and libbpmi.so (device
    memory from bpmi_malloc, inputs built with bpmi_ec_mul_batch_dev) runs an MSM of 2^16 pairs and
    checks it against the known answer -- the C-ABI is sufficient on its own."""
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(repo, "python-bulletproofs_amd")
    exe = str(tmp_path / "msm_c_abi")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-I", os.path.join(repo, "include"), os.path.join(repo, "examples", "msm_c_abi.c"),
                           "-o", exe, os.path.join(libdir, "libbpmi.so"), "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"])
    r = subprocess.run([exe, "16"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "known-answer ok" in r.stdout, r.stdout + r.stderr


def test_async_pair_state_machine(gp):
    """bpmi_msm_dev_enqueue / bpmi_msm_finish: slots, state errors, and the synchronous entry points while a slot is pending."""
    eng = gp.engine()
    lib, ctx = eng.lib, eng.ctx
    pts, _ = gp.rand_points(6000, 91)
    pb, sb = cbind.pack_points(pts), cbind.pack_scalars(list(range(1, 6001)))
    d_p, d_s = eng.upload(pb), eng.upload(sb)
    out = ctypes.create_string_buffer(64)
    want = cbind.msm_bytes(pb, sb, 6000)
    assert lib.bpmi_msm_finish(ctx, 0, out) == -5                       # nothing enqueued
    assert lib.bpmi_msm_dev_enqueue(ctx, 3, d_p.ptr, d_s.ptr, 10) == -3   # no such slot (0, 1, 2 exist)
    assert lib.bpmi_msm_dev_enqueue(ctx, 0, d_p.ptr, d_s.ptr, (1 << 23) + 1) == -3
    assert lib.bpmi_msm_dev_enqueue(ctx, 0, d_p.ptr, d_s.ptr, 6000) == 0
    assert lib.bpmi_msm_dev_enqueue(ctx, 0, d_p.ptr, d_s.ptr, 6000) == -5      # slot still pending
    assert lib.bpmi_msm_dev(ctx, d_p.ptr, d_s.ptr, 6000, out) == -5            # the synchronous call needs slot 0
    assert b"pending" in lib.bpmi_last_error(ctx)
    assert lib.bpmi_msm_dev_enqueue(ctx, 1, d_p.ptr, d_s.ptr, 0) == 0          # n = 0 in the other slot
    assert lib.bpmi_msm_finish(ctx, 0, out) == 0 and out.raw == want
    assert lib.bpmi_msm_finish(ctx, 1, out) == 0 and out.raw == bytes(64)
    assert lib.bpmi_msm_finish(ctx, 1, out) == -5
    assert lib.bpmi_msm_dev(ctx, d_p.ptr, d_s.ptr, 6000, out) == 0 and out.raw == want
    # a synchronous PAIR that is refused because slot 1 holds the caller's asynchronous MSM must leave that MSM alone: its
    # finish returns ITS result (an emptied slot would read as the identity -- "valid" to a verifier) -- ADVICE r03
    o0, o1 = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    assert lib.bpmi_msm_dev_enqueue(ctx, 1, d_p.ptr, d_s.ptr, 6000) == 0
    assert lib.bpmi_msm2(ctx, pb, sb, 6000, o0, pb, sb, 6000, o1) == -5
    assert b"pending" in lib.bpmi_last_error(ctx)
    assert lib.bpmi_msm_finish(ctx, 1, out) == 0 and out.raw == want
    assert lib.bpmi_msm2(ctx, pb, sb, 6000, o0, pb, sb, 6000, o1) == 0 and o0.raw == want and o1.raw == want
    # ... and the same with slot 0 taken: the pair is refused before anything of it is queued
    assert lib.bpmi_msm_dev_enqueue(ctx, 0, d_p.ptr, d_s.ptr, 6000) == 0
    assert lib.bpmi_msm2(ctx, pb, sb, 6000, o0, pb, sb, 6000, o1) == -5
    assert lib.bpmi_msm_finish(ctx, 0, out) == 0 and out.raw == want
    # the third slot; three MSMs in flight, finished out of order
    for sl in (0, 1, 2):
        assert lib.bpmi_msm_dev_enqueue(ctx, sl, d_p.ptr, d_s.ptr, 6000 - sl) == 0
    for sl in (2, 0, 1):
        assert lib.bpmi_msm_finish(ctx, sl, out) == 0 and out.raw == cbind.msm_bytes(pb[:64 * (6000 - sl)], sb[:32 * (6000 - sl)], 6000 - sl)
    eng.set_option("async_lanes", 1)                    # ... and on three lanes
    try:
        for sl in (0, 1, 2):
            assert lib.bpmi_msm_dev_enqueue(ctx, sl, d_p.ptr, d_s.ptr, 6000 - sl) == 0
        for sl in (1, 2, 0):
            assert lib.bpmi_msm_finish(ctx, sl, out) == 0 and out.raw == cbind.msm_bytes(pb[:64 * (6000 - sl)], sb[:32 * (6000 - sl)], 6000 - sl)
    finally:
        eng.set_option("async_lanes", 0)
    # three device segments in one MSM; argument errors
    P = (ctypes.c_void_p * 3)(d_p.ptr, d_p.ptr + 64 * 1000, d_p.ptr + 64 * 2500)
    S = (ctypes.c_void_p * 3)(d_s.ptr, d_s.ptr + 32 * 1000, d_s.ptr + 32 * 2500)
    N = (ctypes.c_uint64 * 3)(1000, 1500, 3500)
    assert lib.bpmi_msm_segs_dev(ctx, 3, P, S, N, out) == 0 and out.raw == want
    N0 = (ctypes.c_uint64 * 3)(1000, 0, 0)
    assert lib.bpmi_msm_segs_dev(ctx, 3, P, S, N0, out) == 0 and out.raw == cbind.msm_bytes(pb[:64000], sb[:32000], 1000)
    assert lib.bpmi_msm_segs_dev(ctx, 4, P, S, N, out) == -3
    assert lib.bpmi_msm_segs_dev(ctx, 0, None, None, None, out) == 0 and out.raw == bytes(64)
    d_p.free()
    d_s.free()


def test_set_option_takes_and_refuses_what_the_case_list_says(gp):
    """bpmi_set_option against tests/option_cases.py -- every option at its default, its accepted edges and the nearest refused values:
    the return code and bpmi_last_error.  On a context of its own, every default restored at once; a refused value leaves the message of
    that option, an unknown name its own text."""
    from bulletproofs_amd.engine import Engine
    from option_cases import CASES, UNKNOWN
    eng = Engine()
    lib, ctx = eng.lib, eng.ctx
    try:
        for name, default, good, bad, msg, _ in CASES:
            for v in [default] + good:
                assert lib.bpmi_set_option(ctx, name.encode(), v) == 0, (name, v, lib.bpmi_last_error(ctx))
                assert lib.bpmi_set_option(ctx, name.encode(), default) == 0, (name, default)
            for v in bad:
                assert lib.bpmi_set_option(ctx, name.encode(), v) == -3, (name, v)
                assert lib.bpmi_last_error(ctx).decode() == msg, (name, v)
        for name in UNKNOWN:
            assert lib.bpmi_set_option(ctx, name.encode(), 0) == -3 and lib.bpmi_last_error(ctx).decode() == "unknown option " + name
        assert lib.bpmi_set_option(ctx, None, 0) == -3 and lib.bpmi_set_option(None, b"chunk", 0) == -3
        # the context still works under its restored defaults
        out = ctypes.create_string_buffer(b"\x55" * 64, 64)
        pts, sc = cbind.pack_points(gp.rand_points(3, 5)[0]), cbind.pack_scalars([1, 2, 3])
        assert lib.bpmi_msm(ctx, pts, sc, 3, out) == 0 and out.raw == cbind.msm_bytes(pts, sc, 3)
    finally:
        eng.close()
