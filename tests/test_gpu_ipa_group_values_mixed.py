"""GPU tests of the grouped values of a list of classes of PACKED inner-product proofs of DIFFERENT lengths
(bpmi_ipa_group_values_packed_mixed_dev, include/bpmi.h; csrc/ipa_group_mixed_dev_host.hpp, k_sc_svector_sum_groups_mixed,
k_msm_ipa_group_mixed): every group's value against bpmi_ipa_group_values_packed_dev on that class's rows through a verifier over the
class's prefix under the same explicit weights, byte for byte; the sum of the values against the mixed verify call; the three routes
in one call; flagged proofs; the two-level locate_packed*(classes, group=...) against the single-proof verifiers and the bisection;
the preparation in several rounds; the C ABI through raw ctypes.  The batch provers make the proofs (prover_table_bits = 4), shared
with tests/test_gpu_ipa_packed_mixed.py; the capacity is 2^9 generators whose first 64 are that module's."""
import ctypes
import functools
import random

import pytest

import ipa_packed_ref as PR
import test_gpu_ipa_packed_mixed as M
from helpers import Q
from test_gpu_ipa_packed_mixed import api_classes, class_list, eng_classes, explicit_weights, single_verdicts

pytestmark = pytest.mark.gpu

E_ARG = -3
SEED = bytes(range(60, 92))
ZERO = bytes(64)
K9, N9 = 9, 512
LIST_A = M.LIST_A                                  # (1, 3), (6, 65), (0, 1), (3, 130), (3, 64)
GROUPINGS = [1, 4, [2, 16, 1, 9, 500]]             # k = 0 and 1: several groups in one wave; 500: the clamp; 65 / 16 and 130 / 9: short last groups


@pytest.fixture(scope="module")
def gp():
    import gpu_common
    return gpu_common


@functools.lru_cache(maxsize=None)
def capacity9(scaled):
    """2^9 generators: the 64 of tests/test_gpu_ipa_packed_mixed.py (so that its classes are statements over prefixes of this list too)
    and 448 more; its u; the optional scale continued."""
    C, D = M.capacity(scaled), M.Capacity()
    more = M._points(2 * (N9 - M.N), 9090 + scaled)
    D.g, D.h, D.u = C.g + more[:N9 - M.N], C.h + more[N9 - M.N:], C.u
    D.scale = None if C.scale is None else C.scale + [random.Random(199).randrange(1, Q) for _ in range(N9 - M.N)]
    return D


@functools.lru_cache(maxsize=None)
def make_class9(k, count, protocol, scaled, prefixed, valid):
    """make_class of the sibling module over the prefixes of the 2^9 capacity (k = 8 and 9)."""
    old = M.capacity
    M.capacity = capacity9
    try:
        return M.make_class.__wrapped__(k, count, protocol, scaled, prefixed, valid)
    finally:
        M.capacity = old


class Verifiers:
    """The mixed verifier over the capacity and, on demand, one single-class verifier per prefix length."""

    def __init__(self, gp, scaled):
        from bulletproofs_amd.innerproduct import MixedBatchInnerProductVerifier
        self.gp, self.C, self.single = gp, capacity9(scaled), {}
        self.bv = MixedBatchInnerProductVerifier(self.C.g, self.C.h, h_scale=self.C.scale, engine=gp.engine())

    def prefix(self, k):
        from bulletproofs_amd.innerproduct import BatchInnerProductVerifier
        if k not in self.single:
            n = 1 << k
            self.single[k] = BatchInnerProductVerifier(self.C.g[:n], self.C.h[:n], h_scale=None if self.C.scale is None else self.C.scale[:n], engine=self.gp.engine())
        return self.single[k]

    def release(self):
        for v in [self.bv] + list(self.single.values()):
            v.release()


def mixed_values(V, protocol, pks, groups, weights=None, seed=None):
    bv = V.bv
    groups = groups if isinstance(groups, list) else [groups] * len(pks)
    return V.gp.engine().ipa_group_values_packed_mixed_dev(bv._d[0], bv._d[1], bv.n, protocol, eng_classes(pks), groups, weights, seed, bv._d_scale)


def single_values(V, protocol, pks, groups, ws):
    """The reference: per class, bpmi_ipa_group_values_packed_dev through the verifier over the class's prefix under its slice of ws."""
    groups = groups if isinstance(groups, list) else [groups] * len(pks)
    values, offs, status, at = [], [0], b"", 0
    for pk, group in zip(pks, groups):
        sv = V.prefix(pk.k)
        v, st = V.gp.engine().ipa_group_values_packed_dev(sv._d[0], sv._d[1], sv.n, protocol, *pk.args(), PR.pack_weights(ws[at: at + pk.count]), None, sv._d_scale, group)
        values, status, at = values + v, status + st, at + pk.count
        offs.append(len(values))
    return values, offs, status


def point_sum(values):
    from bulletproofs_amd.ec import Point
    acc = None
    for v in values:
        if v != ZERO:
            p = Point.from_le64(v)
            acc = p if acc is None else acc + p
    return ZERO if acc is None else acc.to_le64()


# ---- 1. and 2. values against the single-class call, their sum against the verify call ------------------------------------------------
VARIANTS = [(2, False, False), (2, True, True), (1, False, False), (1, True, False)]          # protocol, h_scale, prefixes and starts


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "p%d-%s-%s" % (v[0], "scale" if v[1] else "plain", "starts" if v[2] else "nostarts"))
def test_values_equal_the_single_class_call_and_sum_to_the_verify_call(gp, variant):
    """Five classes about arbitrary statements (no value is the identity), k given as 1, 6, 0, 3, 3.  Every group of every grouping,
    the offsets and the statuses; then the sum of the values against `out` of the mixed verify call under the same weights."""
    protocol, scaled, prefixed = variant
    pks = class_list(LIST_A, protocol, scaled, prefixed)
    total = sum(pk.count for pk in pks)
    V = Verifiers(gp, scaled)
    try:
        ws = explicit_weights(protocol, total, 11 + protocol)
        wb = PR.pack_weights(ws)
        out, out_status = gp.engine().ipa_verify_batch_packed_mixed_dev(V.bv._d[0], V.bv._d[1], V.bv.n, protocol, eng_classes(pks), wb, None, V.bv._d_scale)
        assert out_status == bytes(total) and out != ZERO
        for groups in GROUPINGS:
            want, want_off, want_status = single_values(V, protocol, pks, groups, ws)
            got, off, status = mixed_values(V, protocol, pks, groups, wb)
            assert off == want_off and status == want_status == bytes(total), groups
            assert len(got) == len(want) == off[-1]
            for t, (g_, w_) in enumerate(zip(got, want)):
                assert g_ == w_, (groups, t)
            assert ZERO not in got
            assert point_sum(got) == out, groups
        assert off == [0, 2, 7, 8, 23, 24]                     # the list: 3 / 2, 65 / 16, 1, 130 / 9, 64 / 500 -> one group
    finally:
        V.release()


# ---- 3. all three routes in one call ------------------------------------------------------------------------------------------------------
def test_all_three_routes_in_one_call(gp):
    """(8, 5) in groups of 2: the k_msm_mid shape, one block of the sum per row; (9, 3) in groups of 2: two blocks per row; (3, 1 100)
    in groups of 1 055: one MSM per group (replicas of 130 proofs under distinct weights); (3, 130) in groups of 16: the light shape.
    One wrong statement in each class: exactly those groups are non-zero, and every value equals the single-class call's."""
    (base,) = class_list([(3, 130)], 2, False, False, valid=True)
    pks = [make_class9(8, 5, 2, False, False, True).clone(), make_class9(9, 3, 2, False, False, True).clone(), base.subset([i % 130 for i in range(1100)]), base.clone()]
    groups = [2, 2, 1055, 16]
    for pk, i in zip(pks, (3, 0, 1070, 77)):
        PR.mut_p_changed(pk, i, None)
    total = sum(pk.count for pk in pks)
    V = Verifiers(gp, False)
    try:
        ws = explicit_weights(2, total, 31)
        got, off, status = mixed_values(V, 2, pks, groups, PR.pack_weights(ws))
        want, want_off, want_status = single_values(V, 2, pks, groups, ws)
        assert off == want_off == [0, 3, 5, 7, 16] and status == want_status == bytes(total)
        assert got == want
        assert [t for t, v in enumerate(got) if v != ZERO] == [0 + 3 // 2, 3 + 0, 5 + 1070 // 1055, 7 + 77 // 16]
    finally:
        V.release()


# ---- 4. flagged proofs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("protocol", [1, 2])
def test_flagged_proofs_contribute_to_no_group(gp, protocol):
    shape = [(1, 3), (3, 10), (6, 5)]
    pks = [pk.clone() for pk in class_list(shape, protocol, False, False, valid=True)]
    V = Verifiers(gp, False)
    try:
        rnd = random.Random(5)
        tr = bytearray(pks[1].trs[1])
        tr[len(tr) // 2] ^= 1                              # a transcript byte: bit 0, global index 4
        pks[1].trs[1] = bytes(tr)
        PR.mut_l_off_curve(pks[2], 3, rnd)                 # bit 1, global index 16
        flags = [0] * 18
        flags[4], flags[16] = 1, 2
        ws = explicit_weights(protocol, 18, 21)
        wb = PR.pack_weights(ws)
        got, off, status = mixed_values(V, protocol, pks, 4, wb)
        assert off == [0, 1, 4, 6] and list(status) == flags and got == [ZERO] * 6          # the remaining proofs verify
        PR.mut_p_changed(pks[1], 9, None)                  # a wrong statement: exactly its group is non-zero
        got, off, status = mixed_values(V, protocol, pks, 4, wb)
        want, _, want_status = single_values(V, protocol, pks, 4, ws)
        assert list(status) == flags == list(want_status) and got == want
        assert [t for t, v in enumerate(got) if v != ZERO] == [1 + 9 // 4]
        got, _, status = mixed_values(V, protocol, pks, 4, None, SEED)                      # seed-derived weights go by global index: the same verdicts
        assert [t for t, v in enumerate(got) if v != ZERO] == [3] and list(status) == flags
    finally:
        V.release()


# ---- 5. located indices -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("protocol", [1, 2])
def test_located_indices_equal_the_single_proof_verifiers_and_the_bisection(gp, protocol):
    shape = [(1, 3), (6, 9), (3, 24)]                      # global bases 0, 3, 12
    base = class_list(shape, protocol, False, False, valid=True)
    V = Verifiers(gp, False)
    locate = V.bv.locate_packed2 if protocol == 2 else V.bv.locate_packed1
    try:
        rnd = random.Random(8)
        scattered = [pk.clone() for pk in base]
        PR.mut_a_changed(scattered[0], 1, rnd)                 # 1: only the group equation
        PR.mut_xs_changed(scattered[1], 3, rnd)                # 6: bit 0
        PR.mut_l_off_curve(scattered[1], 8, rnd)               # 11: bit 1
        PR.mut_l_replaced_rehashed(scattered[2], 9, rnd)       # 21
        PR.mut_p_changed(scattered[2], 23, None)               # 35
        one_group = [pk.clone() for pk in base]                # every proof of group 2 (of 4) of the last class is wrong
        for i in (8, 9, 10, 11):
            PR.mut_p_changed(one_group[2], i, None)
        for pks, want in ((scattered, [1, 6, 11, 21, 35]), (one_group, [20, 21, 22, 23]), (base, [])):
            singles = [v for pk in pks for v in single_verdicts(False, pk)]
            assert [i for i, ok in enumerate(singles) if not ok] == want
            bisected = locate(api_classes(pks), group=0)
            assert locate(api_classes(pks)) == bisected == want
            for group in (None, 1, 4, [2, 3, 5]):
                assert locate(api_classes(pks), group=group) == want, group
    finally:
        V.release()


# ---- 6. the preparation in several rounds -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("protocol", [1, 2])
def test_values_do_not_depend_on_the_transcript_budget(gp, protocol):
    """bpmi_debug_ipap_t_budget at 1 000 bytes: rounds of 64 proofs per class, so the classes of 130 and 65 proofs take 3 and 2."""
    eng = gp.engine()
    pks = [pk.clone() for pk in class_list(LIST_A, protocol, True, protocol == 2)]
    PR.mut_xs_changed(pks[3], 129, random.Random(2))
    total = sum(pk.count for pk in pks)
    V = Verifiers(gp, True)
    try:
        wb = PR.pack_weights(explicit_weights(protocol, total, 41))
        whole = [mixed_values(V, protocol, pks, groups, wb) for groups in (9, [2, 16, 1, 9, 500])]
        eng.ipap_t_budget(1000)
        try:
            rounds = [mixed_values(V, protocol, pks, groups, wb) for groups in (9, [2, 16, 1, 9, 500])]
        finally:
            eng.ipap_t_budget(0)
        assert rounds == whole
        assert [i for i, s in enumerate(whole[0][2]) if s] == [3 + 65 + 1 + 129] and ZERO not in whole[0][0]
    finally:
        V.release()


# ---- 7. the C ABI alone -----------------------------------------------------------------------------------------------------------------
def test_the_c_abi_through_raw_ctypes(gp):
    from bulletproofs_amd import _native
    from bulletproofs_amd.ec import pack_points
    from bulletproofs_amd.engine import packed_class_array
    eng = gp.engine()
    shape = [(1, 2), (3, 10), (0, 1), (2, 2)]
    pks = class_list(shape, 2, False, False, valid=True)
    V = Verifiers(gp, False)
    bv = V.bv
    try:
        arr, keep, total, _, _ = packed_class_array(2, eng_classes(pks))
        assert total == 15
        VB, SB = 64 * 8, 32                                # 6 groups under (1, 4, 1, 1) and 15 proofs: guard bytes behind both

        def changed(which, **fields):
            new = (_native.IpaPackedClass * len(arr))()
            ctypes.memmove(new, arr, ctypes.sizeof(arr))
            for name, v in fields.items():
                setattr(new[which], name, v)
            return new

        def call(arr=arr, n_classes=4, n_gens=N9, protocol=2, group=(1, 4, 1, 1), d_g=None, values=True, value_off=True, status=True, seed=SEED):
            v_buf, st_buf = ctypes.create_string_buffer(b"\x55" * VB, VB), ctypes.create_string_buffer(b"\x55" * SB, SB)
            offs = (ctypes.c_uint64 * 6)(*[7] * 6)
            grp = None if group is None else (ctypes.c_uint64 * len(group))(*group)
            rc = eng.lib.bpmi_ipa_group_values_packed_mixed_dev(eng.ctx, bv._d[0].ptr if d_g is None else d_g, bv._d[1].ptr, None, n_gens, protocol, n_classes,
                                                                None if arr is None else ctypes.addressof(arr), None if grp is None else ctypes.addressof(grp), None, seed,
                                                                ctypes.cast(v_buf, ctypes.c_void_p) if values else None, ctypes.addressof(offs) if value_off else None,
                                                                ctypes.cast(st_buf, ctypes.c_void_p) if status else None)
            return rc, eng.lib.bpmi_last_error(eng.ctx).decode(), v_buf.raw, list(offs), st_buf.raw

        untouched = (b"\x55" * VB, [7] * 6, b"\x55" * SB)
        down = (ctypes.c_uint64 * 4)(5, 4, 4, 4)
        cases = [
            # what the mixed packed call refuses, with its messages
            ({"n_classes": 0}, "between 1 and 64 classes"),
            ({"n_classes": 65}, "between 1 and 64 classes"),
            ({"arr": None}, "between 1 and 64 classes"),
            ({"protocol": 3}, "protocol must be 1 or 2"),
            ({"n_gens": 48}, "n_gens must be 2^K, K <= 22"),
            ({"n_gens": 4}, "class 1: k must be at most K"),
            ({"arr": changed(1, ab=None)}, "class 1: null argument"),
            ({"arr": changed(3, xs=None)}, "class 3: null argument (xs and LR may be NULL only at k = 0)"),
            ({"arr": changed(1, tr_off=ctypes.addressof(down))}, "class 1: tr_off must not decrease"),
            ({"seed": None}, "class 0: weights or a 32-byte seed"),
            ({"arr": changed(0, n_proofs=(1 << 16) + 1)}, "class 0: between 1 and 2^16 proofs per call"),
            ({"d_g": 0}, "null argument"),
            # its own
            ({"group": None}, "null argument (group)"),
            ({"group": (1, 4, 0, 1)}, "class 2: group must be at least 1"),
            ({"values": False}, "null argument (values, value_off and status)"),
            ({"value_off": False}, "null argument (values, value_off and status)"),
            ({"status": False}, "null argument (values, value_off and status)"),
            ({"arr": changed(1, k=22), "n_gens": 1 << 22, "group": (1, 1, 1, 1)}, "n_groups x 2 n must not exceed 2^26"),          # 10 groups x 2^23 scalars
        ]
        for kw, text in cases:
            rc, msg, v, offs, st = call(**kw)
            assert rc == E_ARG and text in msg and "bpmi_ipa_group_values_packed_mixed_dev" in msg, (text, rc, msg)
            assert (v, offs, st) == untouched, text
        # a group size of 0 on an EMPTY class is not read as an error; every class empty: BPMI_OK, offsets all zero, values untouched
        empty = (_native.IpaPackedClass * 4)()
        rc, _, v, offs, st = call(arr=empty, group=(0, 0, 0, 0))
        assert rc == 0 and v == untouched[0] and offs == [0] * 5 + [7] and st == untouched[2]
        rc, _, v, offs, st = call()                        # the call itself: 2 + 3 + 1 + 2 groups, the rest of the buffers untouched
        assert rc == 0 and offs == [0, 2, 5, 6, 8, 7] and v == bytes(64 * 8) and st == bytes(15) + b"\x55" * (SB - 15)
        rc, _, v, offs, st = call(group=(1 << 40, 4, 1, 2))                                    # the clamp; 6 groups: two values of guard bytes
        assert rc == 0 and offs == [0, 1, 4, 5, 6, 7] and v == bytes(64 * 6) + b"\x55" * 128 and st == bytes(15) + b"\x55" * (SB - 15)
        # level 2: an off-curve generator among the first n_top = 8 is BPMI_E_ARG and leaves 0xFF in every byte of values; one at
        # index n_top is never read
        d_bad = []
        eng.set_option("validate_points", 2)
        try:
            for index, ok in ((8, True), (7, False)):
                raw = bytearray(pack_points(V.C.g))
                raw[64 * index + 32] ^= 1
                d_bad.append(eng.upload(bytes(raw)))
                rc, msg, v, offs, st = call(d_g=d_bad[-1].ptr, group=(1 << 40, 4, 1, 2))
                if ok:
                    assert rc == 0 and v == bytes(64 * 6) + b"\x55" * 128
                else:
                    assert rc == E_ARG and "d_g[7] is not a point of the curve" in msg and v == b"\xff" * (64 * 6) + b"\x55" * 128
        finally:
            eng.set_option("validate_points", 1)
            for d in d_bad:
                d.free()
        del keep
    finally:
        V.release()
