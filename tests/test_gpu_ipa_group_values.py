"""GPU tests of the grouped verifier of PACKED inner-product proofs (bpmi_ipa_group_values_packed_dev, include/bpmi.h;
csrc/ipa_group_dev_host.hpp, k_sc_svector_sum_groups, k_msm_ipa_group): every group's value against bpmi_ipa_verify_batch_packed_dev
over the rows of that group under the same explicit weights, byte for byte; flagged proofs; the two-level locate_packed* against the
single-proof verifiers and against the bisection; both route switches; the C ABI through raw ctypes; the preparation in several
rounds.  The batch prover makes the proofs (prover_table_bits = 4), shared with tests/test_gpu_ipa_packed.py."""
import ctypes
import functools
import random

import pytest

import ipa_packed_ref as PR
from test_gpu_ipa_packed import explicit_weights, make_batch, make_verifier, packed_out, single_verdicts

pytestmark = pytest.mark.gpu

E_ARG = -3
SEED = bytes(range(60, 92))
ZERO = bytes(64)


@pytest.fixture(scope="module")
def gp():
    import gpu_common
    return gpu_common


def group_values(gp, bv, pk, group, weights=None, seed=None):
    return gp.engine().ipa_group_values_packed_dev(bv._d[0], bv._d[1], bv.n, pk.protocol, *pk.args(), weights, seed, bv._d_scale, group)


def sub_batch_values(gp, bv, pk, ws, group, keep=None):
    """The reference: one verify call per group over the rows of that group (keep: only those of them) under the same weights."""
    group = min(group, pk.count)
    values, status = [], b""
    for lo in range(0, pk.count, group):
        idx = list(range(lo, min(lo + group, pk.count)))
        out, st = packed_out(gp, bv, pk.subset(idx), PR.pack_weights([ws[i] for i in idx]))
        status += st
        if keep is not None:
            idx = [i for i in idx if i in keep]
            out = packed_out(gp, bv, pk.subset(idx), PR.pack_weights([ws[i] for i in idx]))[0] if idx else ZERO
        values.append(out)
    return values, status


# ---- 1. group values equal sub-batch calls --------------------------------------------------------------------------------------------
GROUPS = [1, 4, 9, 16, 130, 500]           # 130 is no multiple of 4, 9 or 16: a short last group; 500: the clamp
VARIANTS = [(2, False, False), (2, True, True), (1, False, False), (1, True, False)]          # protocol, h_scale, prefixes and starts


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "p%d-%s-%s" % (v[0], "scale" if v[1] else "plain", "starts" if v[2] else "nostarts"))
@pytest.mark.parametrize("k", [0, 1, 3, 6])
def test_group_values_equal_the_verify_call_over_each_groups_rows(gp, k, variant):
    """130 proofs about arbitrary statements (every value is a non-trivial point).  k = 0 and k = 1: several groups share a wave of the
    grouped sum.  Every group of every size is compared, and the statuses."""
    protocol, scaled, prefixed = variant
    B = make_batch(k, 130, protocol, scaled, prefixed, False)
    bv = make_verifier(gp, B)
    try:
        ws = explicit_weights(B.pk, 11 * k + protocol)
        wb = PR.pack_weights(ws)
        for group in GROUPS:
            want, want_status = sub_batch_values(gp, bv, B.pk, ws, group)
            got, status = group_values(gp, bv, B.pk, group, wb)
            assert len(got) == len(want) == (130 + min(group, 130) - 1) // min(group, 130)
            assert status == want_status == bytes(130), group
            for t, (g_, w_) in enumerate(zip(got, want)):
                assert g_ == w_, (group, t)
            assert ZERO not in got
    finally:
        bv.release()


# ---- 2. the rows cross blocks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 9])
def test_rows_of_one_and_two_blocks(gp, k):
    """n = 256: one block of the grouped sum per row; n = 512: two.  5 proofs in groups of 2 (a short last group), the k_msm_mid shape."""
    for protocol, scaled in ((2, True), (1, False)):
        B = make_batch(k, 5, protocol, scaled, False, False)
        bv = make_verifier(gp, B)
        try:
            ws = explicit_weights(B.pk, k)
            want, _ = sub_batch_values(gp, bv, B.pk, ws, 2)
            got, status = group_values(gp, bv, B.pk, 2, PR.pack_weights(ws))
            assert got == want and len(got) == 3 and status == bytes(5) and ZERO not in got
        finally:
            bv.release()


# ---- 3. flagged proofs drop out -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("protocol", [1, 2])
def test_flagged_proofs_contribute_to_no_group(gp, protocol):
    B = make_batch(3, 10, protocol, False, False, True)
    bv = make_verifier(gp, B)
    try:
        rnd = random.Random(5)
        pk = B.pk.clone()
        tr = bytearray(pk.trs[1])
        tr[len(tr) // 2] ^= 1                              # a transcript byte: bit 0
        pk.trs[1] = bytes(tr)
        PR.mut_l_off_curve(pk, 6, rnd)                     # bit 1
        ws = explicit_weights(pk, 21)
        wb = PR.pack_weights(ws)
        keep = set(range(10)) - {1, 6}
        got, status = group_values(gp, bv, pk, 4, wb)
        assert list(status) == [0, 1, 0, 0, 0, 0, 2, 0, 0, 0]
        want, want_status = sub_batch_values(gp, bv, pk, ws, 4, keep)
        assert status == want_status and got == want == [ZERO] * 3           # the remaining proofs verify
        PR.mut_p_changed(pk, 9, rnd)                       # a wrong statement: exactly its group is non-zero
        got, status = group_values(gp, bv, pk, 4, wb)
        want, _ = sub_batch_values(gp, bv, pk, ws, 4, keep)
        assert list(status) == [0, 1, 0, 0, 0, 0, 2, 0, 0, 0] and got == want and got[:2] == [ZERO] * 2 and got[2] != ZERO
        # seed-derived weights go by batch index: the same verdicts
        got, status = group_values(gp, bv, pk, 4, None, SEED)
        assert [v == ZERO for v in got] == [True, True, False] and list(status) == [0, 1, 0, 0, 0, 0, 2, 0, 0, 0]
    finally:
        bv.release()


# ---- 4. located indices -------------------------------------------------------------------------------------------------------------------
def locate_packed(bv, pk, group):
    if pk.protocol == 2:
        return bv.locate_packed2(bytes(pk.u), bytes(pk.P), pk.ab, pk.xs, pk.lr, pk.trs, pk.starts, group=group)
    return bv.locate_packed1(bytes(pk.u), bytes(pk.P), bytes(pk.c), pk.ab, pk.xs, pk.lr, pk.head, pk.trs, group=group)


@functools.lru_cache(maxsize=None)
def base_verdicts(protocol):
    """Verifier2 / Verifier1 on every proof of the unchanged batch, once."""
    import gpu_common
    B = make_batch(3, 130, protocol, False, False, True)
    return tuple(single_verdicts(gpu_common, B, B.pk))


def verdicts_after(gp, B, pk, touched):
    """Proof by proof: a proof's verdict depends on its own bytes alone, so only the changed ones are verified again."""
    out = list(base_verdicts(pk.protocol))
    touched = sorted(touched)
    for i, v in zip(touched, single_verdicts(gp, B, pk.subset(touched))):
        out[i] = v
    return out


@pytest.mark.parametrize("protocol", [1, 2])
def test_located_indices_equal_the_single_proof_verifiers_and_the_bisection(gp, protocol):
    B = make_batch(3, 130, protocol, False, False, True)
    bv = make_verifier(gp, B)
    try:
        assert base_verdicts(protocol) == (True,) * 130
        rnd = random.Random(8)
        scattered = B.pk.clone()
        PR.mut_a_changed(scattered, 1, rnd)
        PR.mut_xs_changed(scattered, 3, rnd)                   # bit 0
        PR.mut_l_off_curve(scattered, 6, rnd)                  # bit 1
        PR.mut_l_replaced_rehashed(scattered, 9, rnd)
        one_group = B.pk.clone()                               # every proof of group 2 (of 4) is wrong
        for i in (8, 9, 10, 11):
            PR.mut_p_changed(one_group, i, rnd)
        for pk, touched in ((scattered, {1, 3, 6, 9}), (one_group, {8, 9, 10, 11}), (B.pk, set())):
            want = [i for i, ok in enumerate(verdicts_after(gp, B, pk, touched)) if not ok]
            assert want == sorted(touched)
            bisected = locate_packed(bv, pk, 0)
            for group in (None, 1, 4):
                assert locate_packed(bv, pk, group) == want == bisected, group
    finally:
        bv.release()


# ---- 5. either side of the route switches ---------------------------------------------------------------------------------------------------
def test_either_side_of_both_route_switches(gp):
    """k = 3 under Protocol 2: 16 + 8 group pairs.  62 | 63: the light shape | the k_msm_mid shape; 1 054 | 1 055: that | one MSM per group.
    1 100 proofs (replicas of 130 under distinct weights), one wrong statement."""
    B = make_batch(3, 130, 2, False, False, True)
    bv = make_verifier(gp, B)
    try:
        pk = B.pk.subset([i % 130 for i in range(1100)])
        PR.mut_p_changed(pk, 700, None)
        ws = explicit_weights(pk, 31)
        wb = PR.pack_weights(ws)
        for group in (62, 63, 1054, 1055):
            want, want_status = sub_batch_values(gp, bv, pk, ws, group)
            got, status = group_values(gp, bv, pk, group, wb)
            assert got == want and status == want_status == bytes(1100), group
            assert [t for t, v in enumerate(got) if v != ZERO] == [700 // group], group
    finally:
        bv.release()


# ---- 6. the C ABI alone -----------------------------------------------------------------------------------------------------------------
def test_the_c_abi_through_raw_ctypes(gp):
    from bulletproofs_amd.ec import pack_points
    from bulletproofs_amd.engine import packed_proof_args
    eng = gp.engine()
    B = make_batch(3, 10, 2, False, False, True)
    bv = make_verifier(gp, B)
    try:
        args = list(packed_proof_args(*B.pk.args()))

        def call(args=args, n=8, count=10, group=4, d_g=None, values=True, status=True, seed=SEED):
            v_buf, st_buf = ctypes.create_string_buffer(b"\x55" * 256, 256), ctypes.create_string_buffer(b"\x55" * 16, 16)
            rc = eng.lib.bpmi_ipa_group_values_packed_dev(eng.ctx, bv._d[0].ptr if d_g is None else d_g, bv._d[1].ptr, None, n, 2, count, *args, None, seed, group,
                                                          ctypes.cast(v_buf, ctypes.c_void_p) if values else None, ctypes.cast(st_buf, ctypes.c_void_p) if status else None)
            return rc, eng.lib.bpmi_last_error(eng.ctx).decode(), v_buf.raw, st_buf.raw

        untouched = (b"\x55" * 256, b"\x55" * 16)
        rc, _, v, st = call(args=[None] * 10, count=0)                 # n_proofs = 0: BPMI_OK, nothing is touched
        assert rc == 0 and (v, st) == untouched
        cases = [
            ({"group": 0}, "group must be at least 1"),
            ({"values": False}, "null argument"),
            ({"status": False}, "null argument"),
            ({"n": 1 << 22, "group": 1}, "2^26"),                      # 10 groups x 2^23 scalars
            ({"d_g": 0}, "null argument"),
            ({"seed": None}, "weights or a 32-byte seed"),             # what the packed verifier refuses
            ({"count": (1 << 16) + 1}, "between 1 and 2^16 proofs per call"),
            ({"n": 12}, "n must be 2^k, k <= 22"),
        ]
        for kw, text in cases:
            rc, msg, v, st = call(**kw)
            assert rc == E_ARG and text in msg and "bpmi_ipa_group_values_packed_dev" in msg, (text, rc, msg)
            assert (v, st) == untouched, text
        rc, _, v, st = call()                                          # the call itself: three groups, the rest of the buffer untouched
        assert rc == 0 and v == bytes(192) + b"\x55" * 64 and st == bytes(10) + b"\x55" * 6
        rc, _, v, _ = call(group=1 << 40)                              # the clamp: one group
        assert rc == 0 and v == bytes(64) + b"\x55" * 192
        # level 2: an off-curve generator is BPMI_E_ARG and leaves 0xFF in every byte of values
        raw = bytearray(pack_points(B.g))
        raw[64 * 3 + 32] ^= 1
        d_bad = eng.upload(bytes(raw))
        eng.set_option("validate_points", 2)
        try:
            rc, msg, v, _ = call(d_g=d_bad.ptr)
            assert rc == E_ARG and "d_g[3] is not a point of the curve" in msg and v == b"\xff" * 192 + b"\x55" * 64
            rc, _, v, st = call()
            assert rc == 0 and v == bytes(192) + b"\x55" * 64 and st == bytes(10) + b"\x55" * 6
        finally:
            eng.set_option("validate_points", 1)
            d_bad.free()
    finally:
        bv.release()


# ---- 7. the preparation in several rounds -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("protocol", [1, 2])
def test_values_do_not_depend_on_the_transcript_budget(gp, protocol):
    """bpmi_debug_ipap_t_budget at 1 000 bytes: rounds of 64 proofs, so 130 proofs are prepared in three launches."""
    eng = gp.engine()
    B = make_batch(3, 130, protocol, False, False, True)
    bv = make_verifier(gp, B)
    try:
        pk = B.pk.clone()
        PR.mut_a_changed(pk, 70, None)
        PR.mut_xs_changed(pk, 129, random.Random(2))
        wb = PR.pack_weights(explicit_weights(pk, 41))
        whole = [group_values(gp, bv, pk, group, wb) for group in (9, 130)]
        eng.ipap_t_budget(1000)
        try:
            rounds = [group_values(gp, bv, pk, group, wb) for group in (9, 130)]
        finally:
            eng.ipap_t_budget(0)
        assert rounds == whole
        values, status = whole[0]
        assert [t for t, v in enumerate(values) if v != ZERO] == [70 // 9] and [i for i, s in enumerate(status) if s] == [129]
    finally:
        bv.release()
