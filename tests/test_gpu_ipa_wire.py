"""GPU tests of the wire format BPIP2 of Protocol-2 inner-product proofs (include/bpmi.h; csrc/ipa_wire_kernels.hpp): the device
expansion against its host twin byte for byte (bpmi_ipa_wire_expand_dev / bpmi_ipa_wire_expand) and against the packed arrays the
prover wrote, the decimal writer at its edges, identity points, the whole call (bpmi_ipa_verify_batch_wire_dev) against
bpmi_ipa_verify_batch_packed_dev on the expansion -- same `out`, same status bytes -- for valid, mutated and malformed proofs, several
launches under a small T budget, and the argument errors.  The batch prover makes the proofs (prover_table_bits = 4: small tables).
The expected status bits and texts come from the format's definition, never from the code under test."""
import ctypes
import functools
import os
import random
import subprocess

import pytest

import ipa_wire_common as W
from helpers import Q

pytestmark = pytest.mark.gpu

E_ARG = -3
# the wire prefix lengths of a batch, differing per proof: the word boundaries of the TWriter (7, 8, 9), the SHA-256 block edges of the
# roles behind it (55, 56, 63, 64, 65) and 119; 0 is an empty prefix (start 0), which no prover writes: set by hand
PREFIX_LENS = (1, 7, 8, 9, 55, 56, 63, 64, 65, 119)


@pytest.fixture(scope="module")
def gp():
    import gpu_common
    return gpu_common


def prover_transcript(length):
    """The `transcript` argument under which the prover's prefix -- "&" plus the argument -- has `length` bytes and ends an item."""
    return b"" if length == 1 else b"p" * (length - 2) + b"&"


class Batch:
    """Generators, statements, the packed proofs of one prover call and their blobs."""


@functools.lru_cache(maxsize=None)
def make_batch(k, count, zero=False):
    import gpu_common as gp
    from bulletproofs_amd.ec import secp256k1, unpack_points
    from bulletproofs_amd.innerproduct import BatchInnerProductProver
    from bulletproofs_amd.innerproduct.codec import wire_from_packed
    from bulletproofs_amd.utils import ModP
    n = 1 << k
    eng = gp.engine()
    rnd = random.Random(500 + 10 * k + count)
    ks = b"".join(rnd.randrange(1, Q).to_bytes(32, "little") for _ in range(2 * n + 1))
    pts = unpack_points(eng.ec_mul_batch_bytes(secp256k1.G.to_le64() * (2 * n + 1), ks, 2 * n + 1), 2 * n + 1)
    B = Batch()
    B.k, B.n, B.count = k, n, count
    B.g, B.h, B.u = pts[:n], pts[n: 2 * n], pts[2 * n]
    vec = lambda: [[ModP(0 if zero else rnd.randrange(Q), Q) for _ in range(n)] for _ in range(count)]
    As, Bs = vec(), vec()
    B.prefix_lens = [PREFIX_LENS[i % len(PREFIX_LENS)] for i in range(count)]
    args = [prover_transcript(L) for L in B.prefix_lens]
    eng.set_option("prover_table_bits", 4)
    try:
        bp = BatchInnerProductProver(B.g, B.h, B.u)
        try:
            B.ab, B.xs, B.lr, B.trs = bp.prove2_packed(As, Bs, args)
            B.P = bp.commit_packed(As, Bs, "inner")                      # the statements under which the proofs verify
            B.wire = bp.prove2_wire(As, Bs, args)
        finally:
            bp.close()
    finally:
        eng.set_option("prover_table_bits", 0)
    B.us = B.u.to_le64() * count
    B.starts = [len(t.split(b"&")) if t else 1 for t in args]
    data, off = wire_from_packed(B.ab, B.xs, B.lr, B.trs, B.starts)
    B.blobs = [data[off[i]: off[i + 1]] for i in range(count)]
    return B


def joined(blobs):
    off = [0]
    for b in blobs:
        off.append(off[-1] + len(b))
    return b"".join(blobs), off


def host_expand(k, blobs):
    from bulletproofs_amd.innerproduct.codec import packed_from_wire
    return packed_from_wire(*joined(blobs), k)


def dev_expand(gp, k, blobs):
    return gp.engine().ipa_wire_expand_dev(k, *joined(blobs))


NAMES = ("ab", "xs", "lr", "transcripts", "starts", "status")


def assert_same_expansion(gp, k, blobs):
    want, got = host_expand(k, blobs), dev_expand(gp, k, blobs)
    for name, w_, g_ in zip(NAMES, want, got):
        assert g_ == w_, name
    return want


# ---- 1. the expansion against the host twin and against the prover's arrays ----------------------------------------------------------
@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("k", [0, 1, 3, 6])
def test_expansion_equals_the_host_twin_and_the_provers_arrays(gp, k, count):
    B = make_batch(k, 130)
    blobs = list(B.blobs[:count])
    assert [len(b) for b in blobs] == [78 + 98 * k + L for L in B.prefix_lens[:count]]
    ab, xs, lr, trs, starts, status = assert_same_expansion(gp, k, blobs)
    assert status == bytes(count)
    assert (ab, xs, lr, trs, starts) == (B.ab[: 64 * count], B.xs[: 32 * k * count], B.lr[: 128 * k * count], B.trs[:count], B.starts[:count])
    # every tenth proof with an EMPTY prefix (start 0) and the one behind it with a prefix across two SHA blocks: well formed, no longer valid
    for i in range(0, count, 10):
        blobs[i] = W.with_prefix(blobs[i], k, b"", 0)
        if i + 1 < count:
            blobs[i + 1] = W.with_prefix(blobs[i + 1], k, b"&" + b"q" * 117 + b"&", 2)
    ab, xs, lr, trs, starts, status = assert_same_expansion(gp, k, blobs)
    assert status == bytes(count) and starts[0] == 0 and trs[0] == B.trs[0][B.prefix_lens[0]:]


def test_prove2_wire_writes_the_blobs_of_the_packed_proofs(gp):
    B = make_batch(3, 130)
    data, off = B.wire
    assert [data[off[i]: off[i + 1]] for i in range(B.count)] == B.blobs and list(off)[-1] == len(data)


def test_decimal_writer_edges(gp):
    """x_(k-1) of one blob each set to an edge of the base-10^9 chunks and of the range: the transcript ends with its decimal."""
    k = 3
    B = make_batch(k, 130)
    values = [0, 1, 10**9 - 1, 10**9, 10**18, Q - 1, Q, 2**256 - 1]
    blobs = [W.with_bytes(B.blobs[i], W.scalar_at(2 + k - 1), v.to_bytes(32, "big")) for i, v in enumerate(values)]
    ab, xs, lr, trs, starts, status = assert_same_expansion(gp, k, blobs)
    assert list(status) == [0, 0, 0, 0, 0, 0, 1, 1]
    for i, v in enumerate(values[:6]):
        assert trs[i].endswith(b"&" + str(v).encode() + b"&") and xs[32 * (k * i + k - 1): 32 * (k * i + k)] == v.to_bytes(32, "little"), v
        assert trs[i][: -len(str(v)) - 1] == B.trs[i][: -len(B.trs[i].split(b"&")[-2]) - 1], v        # nothing else moved
    assert trs[6] == trs[7] == b"" and ab[64 * 6: 64 * 8] == bytes(128)


# ---- 2. the whole call ---------------------------------------------------------------------------------------------------------------
def make_verifier(gp, B):
    from bulletproofs_amd.innerproduct import BatchInnerProductVerifier
    return BatchInnerProductVerifier(B.g, B.h, engine=gp.engine())


def pack_weights(ws):
    return b"".join(int(w).to_bytes(32, "little") for w in ws)


def wire_out(gp, bv, blobs, us, Ps, weights):
    data, off = joined(blobs)
    return gp.engine().ipa_verify_batch_wire_dev(bv._d[0], bv._d[1], bv.n, len(blobs), data, off, us, Ps, weights, None)


def packed_out_of_expansion(gp, bv, k, blobs, us, Ps, weights, keep=None):
    """bpmi_ipa_verify_batch_packed_dev over the host twin's expansion (of the proofs `keep`, default all)."""
    ab, xs, lr, trs, starts, _ = host_expand(k, blobs)
    idx = list(range(len(blobs))) if keep is None else keep
    cut = lambda buf, per: b"".join(buf[per * i: per * (i + 1)] for i in idx)
    return gp.engine().ipa_verify_batch_packed_dev(bv._d[0], bv._d[1], bv.n, 2, len(idx), cut(ab, 64), cut(xs, 32 * k), cut(lr, 128 * k), [trs[i] for i in idx],
                                                   [starts[i] for i in idx], cut(us, 64), cut(Ps, 64), None, None, cut(weights, 32), None)


def weights_for(count, seed):
    rnd = random.Random(seed)
    return pack_weights([Q - 1] + [rnd.randrange(1, Q) for _ in range(count - 1)])


def test_identity_points_give_AA_items_and_a_valid_batch(gp):
    k = 3
    B = make_batch(k, 3, zero=True)
    for blob in B.blobs:
        assert blob[W.point_at(k, 0): W.start_at(k)] == bytes(66 * k)
    ab, xs, lr, trs, starts, status = assert_same_expansion(gp, k, B.blobs)
    assert status == bytes(3) and lr == bytes(128 * k * 3) and trs == B.trs and all(t.count(b"AA==&") == 2 * k for t in trs)
    bv = make_verifier(gp, B)
    try:
        ws = weights_for(3, 1)
        out, st = wire_out(gp, bv, B.blobs, B.us, B.P, ws)
        assert (out, st) == packed_out_of_expansion(gp, bv, k, B.blobs, B.us, B.P, ws) and out == bytes(64) and st == bytes(3)
        assert bv.verify_wire2(B.us, B.P, B.blobs) is True
    finally:
        bv.release()


def test_verdicts_equal_the_packed_call_on_the_expansion(gp):
    k, count = 3, 10
    B = make_batch(k, count)
    bv = make_verifier(gp, B)
    ws = weights_for(count, 2)
    flip = lambda b, at: W.with_bytes(b, at, bytes([b[at] ^ 1]))
    mutations = {
        "none": (lambda b: b, 0, True),
        "a": (lambda b: flip(b, W.scalar_at(0) + 31), 0, False),
        "b": (lambda b: flip(b, W.scalar_at(1) + 31), 0, False),
        "x_1": (lambda b: flip(b, W.scalar_at(3) + 31), 1, False),          # the challenge is no longer the re-hash of its prefix
        "prefix_byte": (lambda b: flip(b, W.start_at(k) + 8 + 1), 1, False),
        "tag_parity": (lambda b: flip(b, W.point_at(k, 2)), 1, False),      # a valid encoding of the other point, but x_2 re-hashes its item
    }
    try:
        for name, (mut, want_status, valid) in mutations.items():
            blobs = list(B.blobs)
            blobs[4] = mut(blobs[4])                                         # proof 4: a 55-byte prefix
            out, st = wire_out(gp, bv, blobs, B.us, B.P, ws)
            assert (out, st) == packed_out_of_expansion(gp, bv, k, blobs, B.us, B.P, ws), name
            assert list(st) == [0] * 4 + [want_status] + [0] * 5, name
            assert (out == bytes(64)) == (valid or want_status != 0), name   # a flagged proof contributes nothing; a silent one moves `out`
            assert bv.verify_wire2(B.us, B.P, blobs, weights=[int.from_bytes(ws[32 * i: 32 * i + 32], "little") for i in range(count)]) is valid, name
            data, off = joined(blobs)
            assert bv.verify_wire2(B.us, B.P, data, off) is valid, name
        wrong_P = B.P[:64 * 4] + B.P[64 * 5: 64 * 6] + B.P[64 * 5:]
        out, st = wire_out(gp, bv, B.blobs, B.us, wrong_P, ws)
        assert (out, st) == packed_out_of_expansion(gp, bv, k, B.blobs, B.us, wrong_P, ws) and st == bytes(count) and out != bytes(64)
        assert bv.verify_wire2(B.us, wrong_P, B.blobs) is False
    finally:
        bv.release()


def test_a_flipped_tag_with_its_challenge_rehashed_is_status_0_and_moves_out(gp):
    """The tag's parity flipped is a valid encoding of the other point.  The expansion spells the flipped point in its item, so the
    challenge behind it no longer is the re-hash of its prefix (status bit 0 on both paths: test_verdicts_equal_the_packed_call_on_the_
    expansion).  With that challenge recomputed -- k = 1: R_0 flipped, x_0 = mod_hash of the new prefix, by the oracle -- the proof
    passes every byte-level check, and only the group equation rejects it: status 0, `out` not the identity."""
    from oracle import bp_ref as R
    k = 1
    B = make_batch(k, 130)
    bv = make_verifier(gp, B)
    try:
        blobs = list(B.blobs[:5])
        at = W.point_at(k, 1)                                                # R_0
        b = W.with_bytes(blobs[2], at, bytes([blobs[2][at] ^ 1]))
        tr = host_expand(k, [b])[3][0]
        upto = tr.rindex(b"&", 0, len(tr) - 1) + 1                           # the prefix that ends after R_0's '&'
        x = R.mod_hash(tr[:upto], Q)
        x = int(x.x) if hasattr(x, "x") else int(x)
        blobs[2] = W.with_bytes(b, W.scalar_at(2), x.to_bytes(32, "big"))
        ws = weights_for(5, 3)
        out, st = wire_out(gp, bv, blobs, B.us[:320], B.P[:320], ws)
        assert st == bytes(5) and out != bytes(64)
        assert (out, st) == packed_out_of_expansion(gp, bv, k, blobs, B.us[:320], B.P[:320], ws)
    finally:
        bv.release()


@pytest.mark.parametrize("case", range(8), ids=[name for name, _, _ in W.malformed_table(3)])
def test_a_malformed_blob_alone_among_valid_proofs(gp, case):
    k, count = 3, 5
    B = make_batch(k, 10)
    name, mut, bit = W.malformed_table(k)[case]
    blobs = list(B.blobs[:count])
    blobs[2] = mut(blobs[2])
    us, Ps, ws = B.us[: 64 * count], B.P[: 64 * count], weights_for(count, 4)
    bv = make_verifier(gp, B)
    eng = gp.engine()
    try:
        want_out, want_st = packed_out_of_expansion(gp, bv, k, B.blobs[:count], us, Ps, ws, keep=[0, 1, 3, 4])
        assert want_st == bytes(4) and want_out == bytes(64)
        assert assert_same_expansion(gp, k, blobs)[5] == bytes([0, 0, bit, 0, 0])
        for level in (0, 1, 2):
            eng.set_option("validate_points", level)
            out, st = wire_out(gp, bv, blobs, us, Ps, ws)
            assert list(st) == [0, 0, bit, 0, 0] and out == want_out, (name, level)
        assert bv.verify_wire2(us, Ps, blobs) is False
    finally:
        eng.set_option("validate_points", 1)
        bv.release()


def test_several_launches_give_the_same_bytes(gp):
    """130 proofs under a T budget of one launch of 64: three rounds of expansion, offsets and roles."""
    k, count = 3, 130
    B = make_batch(k, count)
    blobs = list(B.blobs)
    blobs[70] = blobs[70][:-1]                                               # a malformed one in the second round
    blobs[129] = W.with_bytes(blobs[129], W.point_at(k, 0), b"\x04")         # an undecodable point in the third
    bv = make_verifier(gp, B)
    eng = gp.engine()
    ws = weights_for(count, 5)
    try:
        one = wire_out(gp, bv, blobs, B.us, B.P, ws)
        want = host_expand(k, blobs)
        eng.ipap_t_budget(1)                                                 # the plan's floor: 64 proofs per launch
        assert wire_out(gp, bv, blobs, B.us, B.P, ws) == one
        assert dev_expand(gp, k, blobs) == want
    finally:
        eng.ipap_t_budget(0)
        bv.release()
    assert list(one[1]) == [0] * 70 + [1] + [0] * 58 + [2] and one[0] == bytes(64)


def test_argument_errors(gp):
    k, count = 3, 4
    B = make_batch(k, 10)
    bv = make_verifier(gp, B)
    eng = gp.engine()
    lib = eng.lib
    data, off = joined(B.blobs[:count])
    offs = (ctypes.c_uint64 * (count + 1))(*off)
    out, status = ctypes.create_string_buffer(b"\xaa" * 64, 64), ctypes.create_string_buffer(b"\xaa" * count, count)
    seed = bytes(32)

    def call(protocol=2, n_proofs=count, blobs=data, offsets=offs, u=B.us, P=B.P, out_=out, status_=status, n=None):
        return lib.bpmi_ipa_verify_batch_wire_dev(eng.ctx, bv._d[0].ptr, bv._d[1].ptr, None, bv.n if n is None else n, protocol, n_proofs, blobs, offsets, u, P, None, seed,
                                                  ctypes.cast(out_, ctypes.c_void_p), ctypes.cast(status_, ctypes.c_void_p))
    err = lambda: lib.bpmi_last_error(eng.ctx).decode()
    try:
        table = [(dict(protocol=1), "Protocol-2 proofs only"), (dict(protocol=0), "Protocol-2 proofs only"),
                 (dict(offsets=(ctypes.c_uint64 * (count + 1))(0, 500, 400, 900, 1300)), "off must not decrease"),
                 (dict(blobs=None), "null argument"), (dict(offsets=None), "null argument"), (dict(u=None), "null argument"), (dict(P=None), "null argument"),
                 (dict(status_=None), "null argument"), (dict(n_proofs=(1 << 16) + 1), "between 1 and 2^16 proofs per call"), (dict(n=12), "n must be 2^k, k <= 22")]
        for kwargs, msg in table:
            assert call(**kwargs) == E_ARG and msg in err(), (kwargs.keys(), err())
            assert out.raw == b"\xaa" * 64 and status.raw == b"\xaa" * count        # nothing is written on an error
        assert call(out_=None) == E_ARG
        assert call(n_proofs=0) == 0 and out.raw == bytes(64) and status.raw == b"\xaa" * count      # an empty batch: the identity
        assert call() == 0 and out.raw == bytes(64) and status.raw == bytes(count)
        # the expander's hook refuses the same things
        bufs = [ctypes.create_string_buffer(s) for s in (64 * count, 32 * k * count, 128 * k * count, 4096)]
        tr_off, start, st = (ctypes.c_uint64 * (count + 1))(), (ctypes.c_uint32 * count)(), ctypes.create_string_buffer(count)
        xcall = lambda protocol, cap: lib.bpmi_ipa_wire_expand_dev(eng.ctx, k, protocol, count, data, offs, *bufs, cap, tr_off, start, st)
        assert xcall(1, 4096) == E_ARG and "Protocol-2 proofs only" in err()
        assert xcall(2, 16) == E_ARG and "expansion bound" in err()
        assert xcall(2, 4096) == 0 and st.raw == bytes(count)
    finally:
        bv.release()


def test_c_program_proves_encodes_and_verifies_from_bytes_through_the_abi_only(gp, tmp_path):
    """examples/ipa_wire_c_abi.c: a C99 program over include/bpmi.h and libbpmi.so alone proves a batch, encodes it with
    bpmi_ipa_wire_encode, verifies the bytes with bpmi_ipa_verify_batch_wire_dev, and shows both rejections."""
    libdir = os.path.join(W.REPO, "python-bulletproofs_amd")
    exe = str(tmp_path / "ipa_wire_c_abi")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(W.REPO, "include"),
                           os.path.join(W.REPO, "examples", "ipa_wire_c_abi.c"), "-o", exe, os.path.join(libdir, "libbpmi.so"),
                           "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"])
    for args in (["70", "8", "4"], ["3", "1", "4"], ["200", "64", "4"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "(as encoded): VALID" in r.stdout and "(one a changed): INVALID" in r.stdout and "0 proofs flagged" in r.stdout
        if args[1] != "1":
            assert "(one point tag changed): INVALID" in r.stdout and "1 proofs flagged" in r.stdout
