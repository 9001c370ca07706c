"""The wire format BPIP2 of Protocol-2 inner-product proofs on the CPU: the host twin (python-bulletproofs_amd/csrc/ipa_wire_host.hpp)
as a stand-alone program built with the address and undefined-behaviour sanitizers (tests/csrc_host/ipa_wire_host_main.cpp), the
Python codec (innerproduct/codec.py), the pinned encodings of tests/golden/ipa_wire.json and the host entry points of the library.
The yardstick is the reference's own output: every Protocol-2 proof of tests/golden/ipa.json, n = 1 .. 256 -- the plain one (start 1,
prefix "&") and the one inside proof1 (start 3, prefix "&" base64(seed) "&" x "&") -- is encoded and expanded, and the expansion must
be the golden's transcript, challenges, points and start byte for byte; the decompressed y is checked against oracle/ec.py."""
import ctypes
import json
import os
import subprocess

import pytest

import ipa_wire_common as W

REPO = W.REPO
SRC = os.path.join(REPO, "tests", "csrc_host", "ipa_wire_host_main.cpp")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")
FIXTURE = os.path.join(REPO, "tests", "golden", "ipa_wire.json")
E_ARG = -3


def hx(b):
    return bytes(b).hex() or "."


def u64s(vals):
    return b"".join(int(v).to_bytes(8, "little") for v in vals)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ipa_wire_host") / "ipa_wire_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", INC, SRC, "-o", exe])

    def go(texts):
        r = subprocess.run([exe], input="%d\n%s\n" % (len(texts), "\n".join(texts)), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
        lines = [json.loads(line) for line in r.stdout.splitlines()]
        assert len(lines) == len(texts)
        return lines
    return go


def encode_text(k, rows):
    """An E case over packed rows [(ab, xs, lr, transcript, start)]."""
    off = [0]
    for r in rows:
        off.append(off[-1] + len(r[3]))
    arrays = [b"".join(r[0] for r in rows), b"".join(r[1] for r in rows), b"".join(r[2] for r in rows), b"".join(r[3] for r in rows), u64s(off),
              b"".join(int(r[4]).to_bytes(4, "little") for r in rows)]
    return "E %d %d\n%s" % (k, len(rows), "\n".join(hx(a) for a in arrays))


def expand_text(k, blobs):
    off = [0]
    for b in blobs:
        off.append(off[-1] + len(b))
    return "X %d %d\n%s\n%s" % (k, len(blobs), hx(b"".join(blobs)), hx(u64s(off)))


@pytest.fixture(scope="module")
def golden():
    """[(n, name, dict, packed)] of every Protocol-2 proof of the goldens."""
    out = []
    for case in W.golden_cases():
        for name, w2 in W.golden_proofs(case):
            out.append((case["n"], name, w2, W.packed_of(w2)))
    return out


@pytest.fixture(scope="module")
def golden_results(run, golden):
    return run([encode_text(pk[0], [pk[1:]]) for _, _, _, pk in golden])


def test_goldens_cover_n_1_to_256_and_both_prefixes(golden):
    assert sorted({n for n, _, _, _ in golden}) == [1, 2, 4, 8, 16, 32, 64, 128, 256]
    assert {pk[5] for _, _, _, pk in golden} == {1, 3}


def test_host_twin_expands_every_golden_proof_to_the_references_bytes(golden, golden_results):
    for (n, name, w2, (k, ab, xs, lr, tr, start)), res in zip(golden, golden_results):
        what = "n=%d %s" % (n, name)
        assert res["enc_status"] == "00" and res["status"] == "00", what
        blob = bytes.fromhex(res["blobs"])
        prefix = b"&".join(tr.split(b"&")[:start]) + b"&"
        assert len(blob) == 78 + 98 * k + len(prefix) and res["off"] == [0, len(blob)], what
        assert blob == W.blob_of(k, int(w2["a"], 16), int(w2["b"], 16), [int(x, 16) for x in w2["xs"]],
                                 [bytes([2 | (int(p[1], 16) & 1)]) + int(p[0], 16).to_bytes(32, "big") if int(p[0], 16) | int(p[1], 16) else bytes(33)
                                  for p in w2["Ls"] + w2["Rs"]], start, prefix), what
        assert bytes.fromhex(res["tr"]) == tr and res["tr_off"] == [0, len(tr)], what          # the reference's transcript
        assert bytes.fromhex(res["ab"]) == ab and bytes.fromhex(res["xs"]) == xs and res["start"] == [start], what
        assert bytes.fromhex(res["lr"]) == lr, what                                            # the reference's points, y included


def test_decompressed_points_are_the_oracles(golden, golden_results):
    for (n, name, _, (k, *_)), res in zip(golden, golden_results):
        blob, lr = bytes.fromhex(res["blobs"]), bytes.fromhex(res["lr"])
        for j in range(2 * k):
            comp = blob[W.point_at(k, j): W.point_at(k, j) + 33]
            assert lr[64 * j: 64 * j + 64] == W.decompress_oracle(comp), (n, name, j)


def test_python_codec_round_trips_every_golden_proof(golden, golden_results):
    import bulletproofs_amd  # noqa: F401
    from bulletproofs_amd.innerproduct.codec import proof2_to_bytes, proofs2_from_bytes
    for (n, name, w2, _), res in zip(golden, golden_results):
        proof = W.proof2_of(w2)
        blob = proof2_to_bytes(proof)
        assert blob.hex() == res["blobs"], (n, name)                    # the Python codec and the native encoder write the same bytes
        (back,) = proofs2_from_bytes([blob])
        assert (back.a, back.b, back.xs, back.Ls, back.Rs) == (proof.a, proof.b, proof.xs, proof.Ls, proof.Rs), (n, name)
        assert back.transcript == proof.transcript and back.start_transcript == proof.start_transcript, (n, name)


def test_python_codec_refuses_proofs_without_a_wire_form():
    import bulletproofs_amd  # noqa: F401
    from bulletproofs_amd.innerproduct.codec import proof2_from_bytes, proof2_to_bytes
    w2 = W.golden_cases()[3]["proof2"]              # n = 8
    good = W.proof2_of(w2)
    blob = proof2_to_bytes(good)
    for mutate in (lambda p: setattr(p, "transcript", p.transcript + b"tail"),             # trailing text: Verifier2 never reads it
                   lambda p: setattr(p, "transcript", p.transcript + b"&"),
                   lambda p: setattr(p, "start_transcript", p.transcript.count(b"&") + 1),     # fewer '&' than start
                   lambda p: setattr(p, "start_transcript", 2),                                # the rounds do not begin there
                   lambda p: setattr(p, "transcript", p.transcript.replace(b"&", b"&0", 1))):
        bad = W.proof2_of(w2)
        mutate(bad)
        with pytest.raises(ValueError):
            proof2_to_bytes(bad)
    for wrong in (blob[:-1], blob + b"x", b"BPIP1" + blob[5:], W.with_bytes(blob, W.point_at(3, 0), b"\x04"), W.with_bytes(blob, W.scalar_at(0), W.Q.to_bytes(32, "big"))):
        with pytest.raises(ValueError):
            proof2_from_bytes(wrong)


def test_encodings_are_the_pinned_fixture(golden, golden_results):
    """tests/golden/ipa_wire.json was written once by the Python codec (n = 1 and n = 8, both proofs of each): the format must not drift."""
    with open(FIXTURE) as f:
        pinned = json.load(f)
    assert os.path.getsize(FIXTURE) < 10 * 1024
    seen = 0
    for (n, name, _, _), res in zip(golden, golden_results):
        if n in (1, 8):
            assert pinned["n%d.%s" % (n, name)] == res["blobs"], (n, name)
            seen += 1
    assert seen == 4 and len(pinned) == 4


def test_host_twin_flags_each_malformed_blob_alone_among_valid_ones(run, golden, golden_results):
    blobs = {(n, name): bytes.fromhex(res["blobs"]) for (n, name, _, _), res in zip(golden, golden_results)}
    k, good = 3, blobs[(8, "proof1.proof2")]
    table = W.malformed_table(k) + [("a_is_q", lambda b: W.with_bytes(b, W.scalar_at(0), W.Q.to_bytes(32, "big")), 1),
                                    ("x_is_2_256_minus_1", lambda b: W.with_bytes(b, W.scalar_at(2), b"\xff" * 32), 1),
                                    ("prefix_len_lies", lambda b: W.with_bytes(b, W.start_at(k) + 4, (1 << 31).to_bytes(4, "big")), 1),
                                    ("empty", lambda b: b"", 1),
                                    ("expansion_above_2_17", lambda b: W.with_prefix(b, k, b"p" * ((1 << 17) - 3 * 100)), 1)]
    # the mutated blob last too: no read past the end of the buffer (the sanitizer's to report)
    results = run([expand_text(k, [good, mut(good), good]) for _, mut, _ in table] + [expand_text(k, [good, mut(good)]) for _, mut, _ in table])
    ref = run([expand_text(k, [good])])[0]
    for (name, mut, bit), res in zip(table + table, results):
        status = bytes.fromhex(res["status"])
        assert status[0] == 0 and status[1] & bit and status[2:] == bytes(len(status) - 2), name
        assert res["tr_off"][1] == len(bytes.fromhex(ref["tr"])) and bytes.fromhex(res["tr"])[: res["tr_off"][1]] == bytes.fromhex(ref["tr"]), name
        if bit == 1:
            assert res["tr_off"][2] == res["tr_off"][1] and res["start"][1] == 0 and bytes.fromhex(res["ab"])[64:128] == bytes(64), name
        else:
            assert status[1] == 2 and bytes.fromhex(res["lr"])[128 * k: 128 * k + 64] == bytes(64), name       # the one point that does not decode: a zero row


def test_a_flipped_tag_is_a_valid_encoding_of_the_other_point(run, golden_results, golden):
    blobs = {(n, name): bytes.fromhex(res["blobs"]) for (n, name, _, _), res in zip(golden, golden_results)}
    k, good = 3, blobs[(8, "proof2")]
    at = W.point_at(k, 1)
    flipped = W.with_bytes(good, at, bytes([good[at] ^ 1]))
    res = run([expand_text(k, [flipped])])[0]
    assert res["status"] == "00"
    row = bytes.fromhex(res["lr"])[64:128]
    assert row == W.decompress_oracle(flipped[at: at + 33]) and row[32] & 1 == flipped[at] & 1


# ---- the host entry points of the library (no GPU needed: bpmi_ipa_wire_encode / bpmi_ipa_wire_expand take no ctx) ----
@pytest.fixture(scope="module")
def native():
    import bulletproofs_amd  # noqa: F401
    from bulletproofs_amd import _native, build
    build.build()
    return _native.load()


def test_native_encoder_and_expander_agree_with_the_program(native, golden, golden_results):
    from bulletproofs_amd.innerproduct.codec import packed_from_wire, wire_bytes, wire_from_packed
    assert native.bpmi_ipa_wire_bytes(6, 1) == wire_bytes(6, 1) == 78 + 98 * 6 + 1
    by_k = {}
    for (n, name, _, pk), res in zip(golden, golden_results):
        by_k.setdefault(pk[0], []).append((pk, res))
    for k, items in by_k.items():                                   # the two proofs of one n as one batch: prefixes of different lengths
        blobs, off = wire_from_packed(b"".join(pk[1] for pk, _ in items), b"".join(pk[2] for pk, _ in items), b"".join(pk[3] for pk, _ in items),
                                      [pk[4] for pk, _ in items], [pk[5] for pk, _ in items])
        assert blobs.hex() == "".join(res["blobs"] for _, res in items) and list(off)[-1] == len(blobs)
        ab, xs, lr, trs, starts, status = packed_from_wire(blobs, off, k)
        assert status == bytes(len(items)) and trs == [pk[4] for pk, _ in items] and starts == [pk[5] for pk, _ in items]
        assert ab == b"".join(pk[1] for pk, _ in items) and xs == b"".join(pk[2] for pk, _ in items) and lr == b"".join(pk[3] for pk, _ in items)
    k, ab, xs, lr, tr, start = golden[6][3]
    with pytest.raises(ValueError, match="no wire form"):
        wire_from_packed(ab, xs, lr, [tr + b"tail"], [start])
    with pytest.raises(ValueError, match="no wire form"):
        wire_from_packed(ab, xs, lr, [tr], [start + 1])


def test_native_host_calls_refuse_protocol_1_and_bad_arguments(native):
    k, ab, xs, lr, tr, start = W.packed_of(W.golden_cases()[1]["proof2"])          # n = 2
    cap = 78 + 98 * k + len(tr)
    blobs, off, status = ctypes.create_string_buffer(cap), (ctypes.c_uint64 * 2)(), ctypes.create_string_buffer(1)
    tr_off = (ctypes.c_uint64 * 2)(0, len(tr))
    args = lambda protocol, cap_: (k, protocol, 1, ab, xs, lr, tr, tr_off, None, blobs, cap_, off, status)
    err = lambda: native.bpmi_last_error(None).decode()
    assert native.bpmi_ipa_wire_encode(*args(1, cap)) == E_ARG and "Protocol-2 proofs only" in err()
    assert native.bpmi_ipa_wire_encode(*args(2, 10)) == E_ARG and "cap is too small" in err()
    assert native.bpmi_ipa_wire_encode(*args(2, cap)) == 0 and status.raw == b"\x00"
    n = off[1]
    o_ab, o_xs, o_lr, o_tr = (ctypes.create_string_buffer(s) for s in (64, 32 * k, 128 * k, 4096))
    o_off, o_start, o_st = (ctypes.c_uint64 * 2)(), (ctypes.c_uint32 * 1)(), ctypes.create_string_buffer(1)
    xargs = lambda protocol, offs, cap_: (k, protocol, 1, blobs.raw[:n], offs, o_ab, o_xs, o_lr, o_tr, cap_, o_off, o_start, o_st)
    assert native.bpmi_ipa_wire_expand(*xargs(1, off, 4096)) == E_ARG and "Protocol-2 proofs only" in err()
    assert native.bpmi_ipa_wire_expand(*xargs(2, (ctypes.c_uint64 * 2)(5, 4), 4096)) == E_ARG and "off must not decrease" in err()
    assert native.bpmi_ipa_wire_expand(*xargs(2, off, 10)) == E_ARG and "expansion bound" in err()
    assert native.bpmi_ipa_wire_expand(*xargs(2, off, 4096)) == 0 and o_tr.raw[: o_off[1]] == tr and o_start[0] == 1 and o_st.raw == b"\x00"
