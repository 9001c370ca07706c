"""The C-ABI checks the points a caller hands in (option validate_points, default 1): what fastecdsa's Point constructor does for
the reference (reached from /root/reference/src/utils/utils.py:119-131) and ec.py for Python callers, the library does for raw
bytes.  An off-curve point gives BPMI_E_ARG with its index in bpmi_last_error -- never a result."""
import ctypes
import random

import pytest

from helpers import Q
from oracle import cbind
from oracle.ec import secp256k1 as OC

pytestmark = pytest.mark.gpu
P_FIELD = OC.p


@pytest.fixture(scope="module")
def gp():
    import gpu_common
    return gpu_common


def _bad_points():
    """64-byte encodings that are not points: y off by one, x >= p, y >= p, (0, y), only one coordinate zero."""
    G = OC.G
    le = lambda x, y: x.to_bytes(32, "little") + y.to_bytes(32, "little")
    return [le(G.x, G.y + 1), le(G.x + P_FIELD, G.y) if G.x + P_FIELD < (1 << 256) else le(P_FIELD, 1), le(G.x, P_FIELD + 1), le(0, 5), le(G.x, 0),
            le((1 << 256) - 1, (1 << 256) - 1)]


@pytest.mark.parametrize("n", [3, 64, 65, 129, 5000, 70000])
def test_msm_rejects_an_off_curve_point(gp, n):
    eng = gp.engine()
    lib, ctx = eng.lib, eng.ctx
    pts, _ = gp.rand_points(min(n, 500), 7)
    pts = (pts * (n // len(pts) + 1))[:n]
    rnd = random.Random(n)
    sb = cbind.pack_scalars([rnd.randrange(Q) for _ in range(n)])
    good = cbind.pack_points(pts)
    out = ctypes.create_string_buffer(b"\x55" * 64, 64)
    assert lib.bpmi_msm(ctx, good, sb, n, out) == 0 and out.raw == cbind.msm_bytes(good, sb, n)
    for j, bad in enumerate(_bad_points()):
        pos = (j * 7919 + n // 2) % n
        blob = good[: 64 * pos] + bad + good[64 * pos + 64:]
        out = ctypes.create_string_buffer(b"\x55" * 64, 64)
        assert lib.bpmi_msm(ctx, blob, sb, n, out) == -3
        assert b"pts[%d] is not a point of the curve" % pos in lib.bpmi_last_error(ctx)
        assert out.raw == bytes(64)
        # the pair entry point names the array
        o0, o1 = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
        assert lib.bpmi_msm2(ctx, good, sb, n, o0, blob, sb, n, o1) == -3
        assert b"pts1[%d]" % pos in lib.bpmi_last_error(ctx)
    # the identity (64 zero bytes) is a valid input
    blob = bytes(64) + good[64:]
    assert lib.bpmi_msm(ctx, blob, sb, n, out) == 0 and out.raw == cbind.msm_bytes(blob, sb, n)
    # switched off: a result comes back (garbage, as before round 5); switched on again
    try:
        eng.set_option("validate_points", 0)
        blob = good[:64 * (n - 1)] + _bad_points()[0]
        assert lib.bpmi_msm(ctx, blob, sb, n, out) == 0
    finally:
        eng.set_option("validate_points", 1)


def test_dev_entry_points_check_at_level_2(gp):
    eng = gp.engine()
    n = 3000
    pts, _ = gp.rand_points(300, 9)
    good = cbind.pack_points((pts * 10)[:n])
    blob = good[: 64 * 1234] + _bad_points()[0] + good[64 * 1235:]
    sb = cbind.pack_scalars(list(range(1, n + 1)))
    d_p, d_s = eng.upload(blob), eng.upload(sb)
    out = ctypes.create_string_buffer(64)
    try:
        assert eng.lib.bpmi_msm_dev(eng.ctx, d_p.ptr, d_s.ptr, n, out) == 0              # level 1: device pointers are the caller's responsibility
        eng.set_option("validate_points", 2)
        assert eng.lib.bpmi_msm_dev(eng.ctx, d_p.ptr, d_s.ptr, n, out) == -3
        assert b"d_pts[1234]" in eng.lib.bpmi_last_error(eng.ctx) and out.raw == bytes(64)
        d_p.upload(good)
        assert eng.lib.bpmi_msm_dev(eng.ctx, d_p.ptr, d_s.ptr, n, out) == 0 and out.raw == cbind.msm_bytes(good, sb, n)
    finally:
        eng.set_option("validate_points", 1)
        d_p.free(); d_s.free()


def test_other_host_pointer_entry_points(gp):
    eng = gp.engine()
    lib, ctx = eng.lib, eng.ctx
    pts, _ = gp.rand_points(200, 11)
    good = cbind.pack_points(pts)
    bad = _bad_points()[0]
    blob = good[: 64 * 150] + bad + good[64 * 151:]
    sb = cbind.pack_scalars(list(range(1, 201)))
    out = ctypes.create_string_buffer(64 * 200)
    assert lib.bpmi_ec_mul_batch(ctx, blob, sb, 200, out) == -3 and b"pts[150]" in lib.bpmi_last_error(ctx)
    assert out.raw == bytes(64 * 200)                                       # nothing was written
    k = (5).to_bytes(32, "little")
    assert lib.bpmi_ec_lincomb2_batch(ctx, good, blob, k, k, 200, out) == -3 and b"p2[150]" in lib.bpmi_last_error(ctx)
    o64 = ctypes.create_string_buffer(64)
    assert lib.bpmi_ec_sum(ctx, blob, 200, o64) == -3 and b"pts[150]" in lib.bpmi_last_error(ctx)
    assert lib.bpmi_ec_sum(ctx, bad + good[64:640], 10, o64) == -3 and b"pts[0]" in lib.bpmi_last_error(ctx)       # few points: the host-side check
    assert lib.bpmi_ec_sum(ctx, good, 200, o64) == 0
    # inner-product prover: g, h and u
    n = 128
    a = cbind.pack_scalars(list(range(2, n + 2)))
    st = ctypes.c_void_p()
    g, h, u = good[: 64 * n], good[64 * 60: 64 * (60 + n)], good[64 * 199: 64 * 200]
    assert lib.bpmi_ipa_create(ctx, g[: 64 * 17] + bad + g[64 * 18:], h, a, a, n, u, ctypes.byref(st)) == -3 and b"g[17]" in lib.bpmi_last_error(ctx)
    assert lib.bpmi_ipa_create(ctx, g, h[: 64 * 99] + bad + h[64 * 100:], a, a, n, u, ctypes.byref(st)) == -3 and b"h[99]" in lib.bpmi_last_error(ctx)
    assert lib.bpmi_ipa_create(ctx, g, h, a, a, n, bad, ctypes.byref(st)) == -3 and b"u[0]" in lib.bpmi_last_error(ctx)
    assert lib.bpmi_ipa_create_scaled(ctx, g, h[: 64 * 5] + bad + h[64 * 6:], a, a, n, u, a, ctypes.byref(st)) == -3
    assert lib.bpmi_ipa_create(ctx, g, h, a, a, n, u, ctypes.byref(st)) == 0
    lib.bpmi_ipa_destroy(st)
    # the batched prover's generators
    pv = ctypes.c_void_p()
    gs, hs = good[: 64 * 8], good[64 * 8: 64 * 16]
    assert lib.bpmi_rp_prover_create(ctx, 8, u, u, u, gs[: 64 * 3] + bad + gs[64 * 4:], hs, ctypes.byref(pv)) == -3 and b"gs[3]" in lib.bpmi_last_error(ctx)
    assert lib.bpmi_rp_prover_create(ctx, 8, u, bad, u, gs, hs, ctypes.byref(pv)) == -3 and b"h[0]" in lib.bpmi_last_error(ctx)


def _replace(blob, i, point):
    return blob[: 64 * i] + point + blob[64 * (i + 1):]


def test_ipa_verify_dev_names_the_bad_array(gp):
    """bpmi_ipa_verify_dev: up to 64 extra points are checked on the host, before `out` is touched; more by the kernel, and the refused call
    leaves 0xFF.. (never the identity); the generators only from level 2, and of several bad arrays the first in the order d_g, d_h,
    extra_pts is the one named."""
    eng = gp.engine()
    lib, ctx = eng.lib, eng.ctx
    n, k = 4, 2
    pts, _ = gp.rand_points(2 * n + 65, 13)
    g, h, ex = cbind.pack_points(pts[:n]), cbind.pack_points(pts[n: 2 * n]), cbind.pack_points(pts[2 * n:])
    bad = _bad_points()[0]
    xs, xi = cbind.pack_scalars([3, 5]), cbind.pack_scalars([pow(3, -1, Q), pow(5, -1, Q)])
    one, es = cbind.pack_scalars([1]), cbind.pack_scalars(list(range(1, 66)))
    d_g, d_h = eng.upload(g), eng.upload(h)
    fill, refused = b"\x55" * 64, b"\xff" * 64

    def call(ep, ne):
        out = ctypes.create_string_buffer(fill, 64)
        rc = lib.bpmi_ipa_verify_dev(ctx, d_g.ptr, d_h.ptr, None, n, xs, xi, k, one, one, ep, es, ne, out)
        return rc, lib.bpmi_last_error(ctx).decode(), out.raw

    text = "bpmi_ipa_verify_dev: %s is not a point of the curve"
    try:
        for ne in (3, 65):                                                     # well-formed calls (of an invalid statement) on both paths
            rc, _, out = call(ex, ne)
            assert rc == 0 and out not in (fill, refused)
        assert call(_replace(ex, 1, bad), 3) == (-3, text % "extra_pts[1]", fill)          # the host path: `out` keeps its fill pattern
        assert call(_replace(ex, 64, bad), 65) == (-3, text % "extra_pts[64]", refused)      # 65: the smallest count that takes the kernel
        d_g.upload(_replace(g, 3, bad))
        assert call(ex, 3)[0] == 0                                             # level 1: device pointers are the caller's responsibility
        eng.set_option("validate_points", 2)
        assert call(_replace(ex, 64, bad), 65) == (-3, text % "d_g[3]", refused)             # two bad arrays: the one queued first
        d_g.upload(g)
        d_h.upload(_replace(h, 2, bad))
        assert call(ex, 3) == (-3, text % "d_h[2]", refused)
        d_h.upload(h)
        rc, _, out = call(ex, 65)
        assert rc == 0 and out not in (fill, refused)
    finally:
        eng.set_option("validate_points", 1)
        d_g.free(); d_h.free()


def test_batch_verifier_rejects_an_off_curve_commitment(gp):
    """bpmi_rp_batch_verify_dev and bpmi_rp_batch_group_values_dev: a commitment that is not a point is an ARGUMENT error with its index --
    neither a verdict nor a value; from level 2 so is a generator."""
    from bulletproofs_amd.engine import EngineError
    from bulletproofs_amd.rangeproofs import BatchRangeProver, BatchRangeVerifier
    from bulletproofs_amd.utils import ModP, commitment
    from test_gpu_prove_batch import _setup
    n, count = 8, 40
    g, h, gs, hs, u = _setup(gp, n, b"vp")
    rnd = random.Random(8)
    vs = [ModP(rnd.randrange(1 << n), Q) for _ in range(count)]
    gammas = [ModP(rnd.randrange(Q), Q) for _ in range(count)]
    bp = BatchRangeProver(n, g, h, gs, hs, u)
    try:
        blobs = bp.prove_wire(vs, gammas, [b"s%d" % i for i in range(count)])
    finally:
        bp.close()
    Vb = b"".join(commitment(g, h, v, x).to_le64() for v, x in zip(vs, gammas))
    bv = BatchRangeVerifier(g, h, gs, hs, u)
    assert bv.partial_wire(Vb, blobs) == bytes(64)
    with pytest.raises(EngineError, match=r"v_points\[23\] is not a point of the curve"):
        bv.partial_wire(Vb[: 64 * 23] + _bad_points()[0] + Vb[64 * 24:], blobs)
    assert bv.partial_wire(Vb, blobs) == bytes(64)

    # the values of groups of 8 proofs: the same refusal, and every value is left as 0xFF..
    eng = gp.engine()
    bad, group, ngroups = _bad_points()[0], 8, 5

    def group_values(Vs):
        import ctypes as C
        _, cnt, m, src, nbytes, offs, weights, seed, vbytes, d_pts, d_scs = bv._wire_call("group_values_wire", Vs, blobs, None)
        values, status = C.create_string_buffer(b"\x55" * (64 * ngroups), 64 * ngroups), C.create_string_buffer(cnt)
        rc = eng.lib.bpmi_rp_batch_group_values_dev(eng.ctx, n, m, cnt, src, nbytes, C.cast(offs, C.c_void_p), weights, seed, vbytes, bv._d_shared_pts.ptr,
                                                    d_pts.ptr, d_scs.ptr, group, C.cast(values, C.c_void_p), C.cast(status, C.c_void_p))
        return rc, eng.lib.bpmi_last_error(eng.ctx).decode(), values.raw

    text = "bpmi_rp_batch_%s_dev: %s is not a point of the curve"
    refused = b"\xff" * (64 * ngroups)
    assert group_values(Vb)[::2] == (0, bytes(64 * ngroups))
    assert group_values(_replace(Vb, 23, bad)) == (-3, text % ("group_values", "v_points[23]"), refused)
    # level 2: the generators (g, h, u, gs, hs in device memory) are checked too, behind the commitments
    shared = bv._shared_pts
    try:
        eng.set_option("validate_points", 2)
        assert bv.partial_wire(Vb, blobs) == bytes(64)
        bv._d_shared_pts.upload(_replace(shared, 5, bad))
        with pytest.raises(EngineError, match=r"bpmi_rp_batch_verify_dev: d_gens\[5\] is not a point of the curve"):
            bv.partial_wire(Vb, blobs)
        assert group_values(Vb) == (-3, text % ("group_values", "d_gens[5]"), refused)
        with pytest.raises(EngineError, match=r"bpmi_rp_batch_verify_dev: v_points\[23\] is not a point of the curve"):
            bv.partial_wire(_replace(Vb, 23, bad), blobs)
    finally:
        eng.set_option("validate_points", 1)
        bv._d_shared_pts.upload(shared)
    assert bv.partial_wire(Vb, blobs) == bytes(64)
