"""The inputs of tests/transcript_cases.py checked without a GPU: the host twins (bpmi_rp_batch_prepare, engine.ipa_batch_prepare_host:
csrc/rp_batch_host.hpp, ipa_packed_host.hpp, rp_wire_v2_host.hpp -- byte-at-a-time text, pinned to the reference's verifiers elsewhere)
accept every sweep variant, so the inputs are valid by the reference alone; the cover conditions the sweeps exist for are asserted; and
the decimal table's verdicts are the model's.

The cover, computed by transcript_cases.hash_points (conditions, not measurements):
  (a) for every digest point (Protocol 1's challenge, each of the k rounds) the block fill at sha_digest_number, (1 + message length)
      % 64, takes all 64 values over the sweep -- 55 (the padding just fits), 56 (a second block), 63 and 0 among them;
  (b) in the range-proof sweep each of the 64 occurs with each of the 8 values of (blob offset of the transcript) % 8: 512 cells per point;
  (c) every (fill & 3, off & 7) an incremental sha_feed can start at occurs for each round: round 0 always starts behind the "1"
      (fill & 3 = 1) at each of the 8 offsets; every later round starts at all 32 pairs.  In the packed family a transcript is
      transposed from its own byte 0, so there fill & 3 is (off + 1) & 3: 8 pairs per later round, and each of the 8 offsets for
      Protocol 1's challenge.
Final pad sets.  Range proofs: pad0 = 0..7 crossed with pad1 = pad2 = 0..127 and 137, 145, 150, 156, 157, 180, 313 -- 1 080 proofs.  Two
turns of the pad left round 1 without fill 47 and round 2 without fills 4, 12, 17, 23, 44 and 53 (the recomputed x_i change length by
a digit or two); the seven added values fill them.  Packed Protocol 2: b"", None, one-item prefixes of 0..127 and of 182 bytes (round 1
had no fill 59), two-item prefixes for p = 0..15 -- 147 proofs.  Packed Protocol 1: item 0 of 0..7 bytes crossed with item 1 of 0..63
bytes -- 512 proofs, nothing added.

The decimal table: 501 rows, 163 with a value by the model and 338 without; applied to y, z and x that is 487 accepted proofs
(y = "0" and y = str(q) have the value 0 and are refused: ZERO_RULE) and 1 016 refused ones.  The host twin agrees with the model on
every one."""
import functools
import random

import pytest

import ipa_packed_ref as PR
import transcript_cases as TC
from helpers import Q


# ---- the one oracle proof per family --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rp_base():
    """(format 1, format 2, format 3) bytes of test_batch_verify_cpu.make_batch(1, n=8)'s proof."""
    import bulletproofs_amd  # noqa: F401
    from bulletproofs_amd.rangeproofs.codec import proof_to_bytes
    from test_batch_verify_cpu import make_batch
    pr = make_batch(1, n=8)["proofs"][0]
    return tuple(proof_to_bytes(pr, version=v) for v in (1, 2, 3))


@functools.lru_cache(maxsize=None)
def ipa_base(protocol):
    """A one-proof Packed at k = 2 from the oracle's prover."""
    if protocol == 2:
        return PR.oracle_batch2(4, 1, 4242, prefixes=[None])[2]
    return PR.oracle_batch1(4, 1, 4343, [b"seed"])[2]


@functools.lru_cache(maxsize=None)
def rp_sweep():
    return TC.rp_phase_sweep(rp_base()[0])


@functools.lru_cache(maxsize=None)
def ipa_sweep(protocol):
    return TC.ipa2_phase_sweep(ipa_base(2)) if protocol == 2 else TC.ipa1_phase_sweep(ipa_base(1))


def weights_for(count, per, seed):
    rnd = random.Random(seed)
    return b"".join(rnd.randrange(1, Q).to_bytes(32, "little") for _ in range(per * count))


def rp_host(blobs, weights=None, seed=None):
    from test_gpu_batch_dev import host_prepare
    if weights is None and seed is None:
        weights = weights_for(len(blobs), 4, len(blobs))
    return host_prepare(8, 1, blobs, weights, seed)


def ipa_weights(pk, seed):
    rnd = random.Random(seed)
    return [[rnd.randrange(1, Q) for _ in range(3 if pk.protocol == 1 else 1)] for _ in range(pk.count)]


def ipa_host(pk, ws):
    from bulletproofs_amd.engine import ipa_batch_prepare_host
    return ipa_batch_prepare_host(pk.k, pk.protocol, *pk.args(), PR.pack_weights(ws), None, 3)


def assert_ipa_expected(pk, got, ws):
    """records, extra points and extra scalars of every proof against Python integers (ipa_packed_ref.expected)."""
    pairs, rb = PR.pairs_of(pk.k, pk.protocol), 64 * pk.k + 96
    for i in range(pk.count):
        rec, pts, sc = PR.expected(pk, i, ws[i])
        assert (got[0][rb * i: rb * (i + 1)], got[1][64 * pairs * i: 64 * pairs * (i + 1)], got[2][32 * pairs * i: 32 * pairs * (i + 1)]) == (rec, pts, sc), i


# ---- the builders ----------------------------------------------------------------------------------------------------------------------------
def test_the_builders_reproduce_the_oracle_provers_own_hashes():
    """With no padding the builders re-hash every chain and write the bytes the oracle's provers wrote."""
    v1, v2, v3 = rp_base()
    assert TC.rp_v1_variant(v1, 0, 0, 0) == v1
    k, head, start, ts = TC.rp_split(v1)
    assert (k, start) == (3, 3) and TC.rp_join(head, start, ts) == v1
    for j in TC.ROLES:
        assert TC.rp_v1_set_item(v1, j, ts[0].split(b"&")[j]) == v1
    from base64 import b64decode
    seed0, seed1 = b64decode(ts[0].split(b"&")[0]), b64decode(ts[1].split(b"&")[0])
    assert TC.rp_v2_variant(v2, seed0, seed1) == v2
    assert TC.rp_v3_of(v2, TC.v3_ys(v3)) == v3
    pk = ipa_base(2)
    one = TC.ipa_variant(pk, 0, None)
    assert (one.trs, bytes(one.xs), one.starts) == (pk.trs, bytes(pk.xs), [1])
    pk = ipa_base(1)
    items = pk.trs[0].split(b"&")
    one = TC.ipa1_variant(pk, 0, items[0], items[1])
    assert (one.trs, bytes(one.xs)) == (pk.trs, bytes(pk.xs))
    assert len({TC.pattern(64, ph)[i: i + 8] for ph in range(9) for i in range(0, 56)}) > 60 and b"&" not in TC.pattern(200)


# ---- the phase sweeps: valid by the host twins -----------------------------------------------------------------------------------------------
def test_the_host_twin_accepts_every_range_proof_of_the_phase_sweep():
    blobs = rp_sweep()
    assert len(blobs) == len(TC.RP_PAD0) * len(TC.RP_PADS) == 1080 and len(set(blobs)) == 1080
    rc, bad = rp_host(blobs)[:2]
    assert (rc, bad) == (0, -1)
    assert rp_host(blobs, None, bytes(range(32)))[:2] == (0, -1)


@pytest.mark.parametrize("protocol", [1, 2])
def test_the_host_twin_accepts_every_packed_proof_of_the_phase_sweep(protocol):
    pk = ipa_sweep(protocol)
    assert pk.count == (512 if protocol == 1 else 2 + 129 + 16)
    ws = ipa_weights(pk, 50 + protocol)
    got = ipa_host(pk, ws)
    assert got[3] == bytes(pk.count)
    assert_ipa_expected(pk, got, ws)


# ---- the cover ---------------------------------------------------------------------------------------------------------------------------------
ALL64 = set(range(64))
ALL_PAIRS = {(f, o) for f in range(4) for o in range(8)}


def test_the_range_proof_sweep_covers_every_block_phase_at_every_alignment():
    cells, feeds = {}, {}
    for blob in rp_sweep():
        for hp in TC.hash_points(blob):
            cells.setdefault(hp["name"], set()).add(((1 + hp["msg_len"]) % 64, hp["ts_off"] % 8))
            feeds.setdefault(hp["name"], set()).add(hp["feed"])
    assert sorted(cells) == ["p1", "round0", "round1", "round2"]
    for name, got in cells.items():
        assert {f for f, _ in got} == ALL64, name                                        # (a)
        assert got == {(f, o) for f in range(64) for o in range(8)}, name                # (b)
    first = {(1, o) for o in range(8)}                                                   # (c)
    assert feeds["p1"] == first and feeds["round0"] == first
    assert feeds["round1"] == ALL_PAIRS and feeds["round2"] == ALL_PAIRS


def test_the_packed_sweeps_cover_every_block_phase():
    fills, feeds = {}, {}
    for protocol in (1, 2):
        pk = ipa_sweep(protocol)
        for tr, s in zip(pk.trs, pk.starts or [3] * pk.count):
            for hp in TC.ipa_hash_points(tr, s, pk.k, protocol):
                fills.setdefault((protocol, hp["name"]), set()).add((1 + hp["msg_len"]) % 64)
                feeds.setdefault((protocol, hp["name"]), set()).add(hp["feed"])
    assert sorted(fills) == [(1, "p1"), (1, "round0"), (1, "round1"), (2, "round0"), (2, "round1")]
    for key, got in fills.items():
        assert got == ALL64, key                                                         # (a)
    locked = {((o + 1) & 3, o) for o in range(8)}                                        # (c)
    assert feeds[(1, "p1")] == {(1, o) for o in range(8)}
    assert feeds[(1, "round0")] == feeds[(2, "round0")] == {(1, 0)}
    assert feeds[(1, "round1")] == locked and feeds[(2, "round1")] == locked


# ---- the decimal table: the host twin against the model -----------------------------------------------------------------------------------------
def test_the_model_on_the_rows_that_name_their_value():
    M, row = TC.decimal_model, TC.DECIMAL_ROW
    assert M(row["q+5"]) == 5 == M(row["5"]) and M(row["q"]) == 0 == M(row["0"]) and M(row["q-1"]) == Q - 1 and M(row["q+1"]) == 1
    assert M(row["2^256-1"]) == 2 ** 256 - 1 - Q and M(row["10^77"]) == 10 ** 77 and M(row["9x77"]) == 10 ** 77 - 1
    for name in ("2^256", "2^256+1", "10^78-1", "10^78", "00", "01", "empty", "trailing-newline"):
        assert M(row[name]) is None, name
    assert M(b"1" * 79) is None and M(b"+5") is None and M(b"5 ") is None and M(b"\xd9\xa3") is None
    valued = [name for name, item in TC.DECIMAL_ROWS if M(item) is not None]
    assert len(TC.DECIMAL_ROWS) == 501 and len(valued) == TC.DECIMAL_VALUED == 163 and 501 - len(valued) == TC.DECIMAL_REFUSED == 338
    assert [TC.ZERO_RULE[j][0] for j in TC.ROLES] == [False, True, True]


def test_the_host_twins_verdict_on_every_decimal_row_is_the_models():
    v1 = rp_base()[0]
    acc, ref = TC.decimal_cases(v1)
    assert len(acc) == 3 * TC.DECIMAL_VALUED - 2 == 487 and len(ref) == 3 * TC.DECIMAL_REFUSED + 2 == 1016
    assert sorted((name, j) for name, j, _ in ref if TC.decimal_model(TC.DECIMAL_ROW[name]) is not None) == [("0", 3), ("q", 3)]
    w = weights_for(3, 4, 9)
    wrong = [(name, j) for name, j, blob in acc if rp_host([v1, blob, v1], w)[:2] != (0, -1)]
    wrong += [(name, j) for name, j, blob in ref if rp_host([v1, blob, v1], w)[:2] != (0, 1)]
    assert wrong == []
    assert rp_host([blob for _, _, blob in acc])[:2] == (0, -1)
    # the value the twin read, where a per-proof scalar shows it: V's is -w1 z^2, T1's is -w1 x (all weights 1 here)
    ones = (1).to_bytes(32, "little") * 4
    for name, j, blob in acc:
        if j != 3:
            got = rp_host([blob], ones)
            v = TC.decimal_model(TC.DECIMAL_ROW[name])
            want = (-v * v) % Q if j == 4 else (-v) % Q
            assert int.from_bytes((got[2] if j == 4 else got[3])[:32], "little") == want, (name, j)
    # a value in [q, 2^256) is reduced: the same bytes as its residue's row
    for j in TC.ROLES:
        for big, small in ((Q + 5, 5), (2 ** 256 - 1, 2 ** 256 - 1 - Q)):
            a = rp_host([TC.rp_v1_set_item(v1, j, str(big).encode())], ones)
            b = rp_host([TC.rp_v1_set_item(v1, j, str(small).encode())], ones)
            assert a[:2] == (0, -1) and a == b, (j, big)


# ---- formats 2 and 3 -------------------------------------------------------------------------------------------------------------------------------
def v2_batches():
    """name -> list of format-2 proofs: the seed sweep and the value sweep of y, z and x."""
    v2 = rp_base()[1]
    out = {"seeds": TC.v2_seed_sweep(v2)}
    for j in range(3):
        out["values-" + "yzx"[j]] = TC.v2_value_sweep(v2, j)
    return out


def test_the_host_twin_takes_every_format_2_variant_as_its_format_1_expansion():
    from bulletproofs_amd.rangeproofs.codec import wire_v2_to_v1
    v1, v2, v3 = rp_base()
    batches = v2_batches()
    assert len(batches["seeds"]) == 50 and all(len(b) == 3 * len(TC.V2_VALUES) == 492 for n, b in batches.items() if n != "seeds")
    for name, blobs in batches.items():
        w = weights_for(len(blobs), 4, len(name))
        got = rp_host(blobs, w)
        assert got[:2] == (0, -1), name
        assert rp_host([wire_v2_to_v1(b) for b in blobs], w) == got, name
    ys = TC.v3_ys(v3)
    v3s = [TC.rp_v3_of(b, ys) for b in batches["seeds"]]
    w = weights_for(len(v3s), 4, 3)
    assert rp_host(v3s, w) == rp_host(batches["seeds"], w)
    # the three base64 tails in front of every byte alignment of the item behind them.  The range-proof transcript starts at a fixed
    # blob offset (664 at k = 3: a multiple of 8) and a seed item is 4 ceil(n / 3) + 1 bytes, so the item behind seed0 starts at 1 or 5
    # mod 8; the Protocol-1 seed, and its copy in the Protocol-2 transcript, sit behind the decimals of y, z, x and meet all 8
    cells = {0: set(), 1: set(), 2: set()}
    for blobs in batches.values():
        for b in blobs:
            k, head, start, ts = TC.rp_split(wire_v2_to_v1(b))
            off0 = len(head) + 6
            off1 = off0 + len(ts[0]) + 4
            off2 = off1 + len(ts[1]) + 4
            seeds = [int.from_bytes(b[len(head) + 128: len(head) + 130], "big")]
            seeds.append(int.from_bytes(b[len(head) + 130 + seeds[0]: len(head) + 132 + seeds[0]], "big"))
            cells[0].add((seeds[0] % 3, (off0 + len(ts[0].split(b"&")[0]) + 1) % 8))
            cells[1].add((seeds[1] % 3, (off1 + len(ts[1].split(b"&")[0]) + 1) % 8))
            cells[2].add((seeds[1] % 3, (off2 + 1 + len(ts[2].split(b"&")[1]) + 1) % 8))
    assert cells[0] == {(t, o) for t in range(3) for o in (1, 5)}
    assert cells[1] == cells[2] == {(t, o) for t in range(3) for o in range(8)}
    for j, v, blob in TC.v2_refused(v2):
        assert rp_host([v2, blob, v2], weights_for(3, 4, 1))[:2] == (0, 1), (j, v)
