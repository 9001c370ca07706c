"""The device's transcript reader against the inputs of tests/transcript_cases.py (validated without a GPU by
tests/test_transcript_cases_cpu.py, which also asserts what they cover): the text-handling code that exists only on the device --
the SHA-256 that defers compression (sha_feed, sha_push_byte / word, sha_digest_number, mod_hash_q), the unaligned loads over the
transposed array (BPtr, ld8), the item walker (first_amp, walk_end), the decimal reader (eight_digits, parse_decimal), the base64 point
compare (point_item_equals, point_item_equals_le) and the format-2/3 expander k_rp_expand_v2 (dec_chunks, dec_item_len, tw_decimal,
tw_b64, tw_store's atomicOr): csrc/rp_batch_kernels.hpp, reused unchanged by csrc/ipa_packed_kernels.hpp -- at every block phase of
every digest point with every alignment of the transcript, on decimals of every length and at the edges of the accepted range, on every
non-digit boundary byte at every position of a chunk, and on every base64 tail in front of every alignment of the next item.  The
device must give the host twin's bytes and verdicts, the model's verdicts (transcript_cases.decimal_model) and, for packed proofs,
the Python integers of ipa_packed_ref.expected.  Every call is one small batch at n = 8 generators (k = 3) or k = 2 (packed).

NOT covered, here or anywhere: the retry of mod_hash (i >= 2: a digest that is zero or not below q).  No input reaches it on either
side (probability about 2^-128 per challenge), and there is no hook for it."""
import pytest

import bulletproofs_amd  # noqa: F401
import transcript_cases as TC
from helpers import Q
from test_gpu_batch_dev import assert_same, dev_prepare, host_prepare
from test_gpu_ipa_packed import dev_prepare as ipa_dev_prepare
from test_gpu_ipa_packed import explicit_weights
from test_gpu_ipa_packed import host_prepare as ipa_host_prepare
from test_transcript_cases_cpu import assert_ipa_expected, ipa_sweep, rp_base, rp_sweep, v2_batches, weights_for

import ipa_packed_ref as PR

pytestmark = pytest.mark.gpu

SEED = bytes(range(40, 72))
ONES = (1).to_bytes(32, "little") * 4


@pytest.fixture(scope="module")
def eng():
    from bulletproofs_amd.engine import default_engine
    return default_engine()


@pytest.fixture(scope="module")
def gp():
    import gpu_common
    return gpu_common


# ---- 1. range proofs, format 1: every block phase of every digest point at every alignment ----------------------------------------------
def test_range_proof_phase_sweep(eng):
    """1 080 variants of one proof (pad0 x pad1 = pad2) in one call with explicit weights and in one with a seed: no proof is called
    bad, and V scalars, per-proof scalars, shared coefficients and decoded points are the host twin's bytes; then with 16 proofs per
    wave and 37 rows per launch, so that proofs of different phases share waves differently."""
    blobs = rp_sweep()
    assert_same(eng, 8, 1, blobs, weights_for(len(blobs), 4, 1), None)
    assert_same(eng, 8, 1, blobs, None, SEED)
    want = host_prepare(8, 1, blobs, None, SEED)
    try:
        eng.set_option("rp_lanes", 16)
        eng.set_option("rp_rows", 37)
        got = dev_prepare(eng, 8, 1, blobs, None, SEED)
    finally:
        eng.set_option("rp_lanes", 0)
        eng.set_option("rp_rows", 0)
    assert got[:5] == want[:5]


# ---- 2. packed inner-product proofs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("protocol", [2, 1])
def test_packed_phase_sweep(gp, protocol):
    """Protocol 2: no prefix, one-item prefixes of 0..127 (and 182) bytes, two-item prefixes; Protocol 1: item 0 of 0..7 bytes x item 1
    of 0..63 bytes.  One call: every status 0; records, extra points and extra scalars are the host twin's and, proof by proof, the
    Python integers of ipa_packed_ref.expected."""
    pk = ipa_sweep(protocol)
    ws = explicit_weights(pk, 60 + protocol)
    weights = PR.pack_weights(ws)
    want, got = ipa_host_prepare(pk, weights), ipa_dev_prepare(gp, pk, weights)
    assert got[3] == bytes(pk.count) and want[3] == bytes(pk.count)
    for name, w_, g_ in zip(("records", "extra_pts", "extra_scalars"), want, got):
        assert g_ == w_, name
    assert_ipa_expected(pk, got, ws)
    assert ipa_dev_prepare(gp, pk, None, SEED) == ipa_host_prepare(pk, None, SEED)


# ---- 3. the decimal reader ---------------------------------------------------------------------------------------------------------------------
def test_decimal_rows_with_a_value_are_read_as_the_model_reads_them(eng):
    """The 487 accepted (row, item) pairs in one call: the host twin's bytes; where a per-proof scalar shows the value read -- V's is
    -w1 z^2, T1's is -w1 x -- it is the model's; a value in [q, 2^256) gives the bytes of its residue."""
    v1 = rp_base()[0]
    acc, ref = TC.decimal_cases(v1)
    assert len(acc) == 3 * TC.DECIMAL_VALUED - 2 == 487 and len(ref) == 3 * TC.DECIMAL_REFUSED + 2 == 1016
    blobs = [blob for _, _, blob in acc]
    assert_same(eng, 8, 1, blobs, weights_for(len(blobs), 4, 2), None)
    got = dev_prepare(eng, 8, 1, blobs, ONES * len(blobs), None)
    assert got[:2] == (0, -1)
    for i, (name, j, _) in enumerate(acc):
        v = TC.decimal_model(TC.DECIMAL_ROW[name])
        if j == 4:
            assert int.from_bytes(got[2][32 * i: 32 * i + 32], "little") == (-v * v) % Q, name
        elif j == 7:
            assert int.from_bytes(got[3][32 * 12 * i: 32 * 12 * i + 32], "little") == (-v) % Q, name
    for j in TC.ROLES:
        for big, small in ((Q + 5, 5), (2 ** 256 - 1, 2 ** 256 - 1 - Q)):
            assert TC.rp_v1_set_item(v1, j, str(big).encode()) in blobs
            a = dev_prepare(eng, 8, 1, [TC.rp_v1_set_item(v1, j, str(big).encode())], ONES, None)
            b = dev_prepare(eng, 8, 1, [TC.rp_v1_set_item(v1, j, str(small).encode())], ONES, None)
            assert a[:2] == (0, -1) and a == b, (j, big)


@pytest.mark.parametrize("j", TC.ROLES, ids=["y", "z", "x"])
def test_decimal_rows_without_a_value_are_refused(eng, j):
    """Each refused row between two good proofs, one call each: the device names proof 1, as the host twin does and the model says."""
    v1 = rp_base()[0]
    ref = [(name, blob) for name, jj, blob in TC.decimal_cases(v1)[1] if jj == j]
    assert len(ref) == TC.DECIMAL_REFUSED + (2 if j == 3 else 0)
    w = weights_for(3, 4, j)
    wrong = []
    for name, blob in ref:
        h = host_prepare(8, 1, [v1, blob, v1], w, None)
        d = dev_prepare(eng, 8, 1, [v1, blob, v1], w, None)
        if (h[0], h[1], d[0], d[1]) != (0, 1, 0, 1):
            wrong.append((name, h[:2], d[:2]))
    assert wrong == []


# ---- 4. the expander, formats 2 and 3 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["seeds", "values-y", "values-z", "values-x"])
def test_expander_writes_what_the_codec_writes(eng, name):
    """Seeds of 0..23 bytes on either side (the three base64 tails in front of every alignment of the next item), two proofs whose
    L_0 is the identity, and y, z, x over short decimals, base-10^9 chunks with interior zeros and q - 1: the device's expansion gives
    what the device gives for codec.wire_v2_to_v1's bytes, and what the host twin gives.  The seed sweep again as format 3."""
    from bulletproofs_amd.rangeproofs.codec import wire_v2_to_v1
    blobs = v2_batches()[name]
    w = weights_for(len(blobs), 4, len(name))
    d2 = dev_prepare(eng, 8, 1, blobs, w, None)
    d1 = dev_prepare(eng, 8, 1, [wire_v2_to_v1(b) for b in blobs], w, None)
    assert d2[:2] == (0, -1) and d2 == d1
    assert_same(eng, 8, 1, blobs, w, None)
    if name == "seeds":
        ys = TC.v3_ys(rp_base()[2])
        v3s = [TC.rp_v3_of(b, ys) for b in blobs]
        assert dev_prepare(eng, 8, 1, v3s, w, None) == d1
        assert_same(eng, 8, 1, v3s, None, SEED)
        assert_same(eng, 8, 1, blobs, None, SEED)


def test_expander_refuses_a_challenge_that_is_not_below_q(eng):
    v2 = rp_base()[1]
    w = weights_for(3, 4, 5)
    for j, v, blob in TC.v2_refused(v2):
        assert host_prepare(8, 1, [v2, blob, v2], w, None)[:2] == (0, 1), (j, v)
        assert dev_prepare(eng, 8, 1, [v2, blob, v2], w, None)[:2] == (0, 1), (j, v)
