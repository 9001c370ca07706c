"""The Python surface of the batched inner-product prover -- innerproduct.BatchInnerProductProver -- where it runs without a GPU: the
argument checks that come before the native call, on a stub engine that records what reaches it
(src/innerproduct/inner_product_prover.py:20-27 and :42-54 are the constructors whose loop it replaces)."""
import ctypes

import pytest

import bulletproofs_amd  # noqa: F401
from bulletproofs_amd.ec import PackedPoints, Point, secp256k1
from bulletproofs_amd.innerproduct import BatchInnerProductProver
from bulletproofs_amd.utils.utils import ModP

Q = secp256k1.q
G = Point._raw(secp256k1.gx, secp256k1.gy)


class StubLib:
    """The five entry points: create hands out a handle, proving must never be reached by a call these tests expect to be refused."""

    def __init__(self):
        self.created, self.destroyed, self.proved = [], [], []

    def bpmi_ipa_batch_prover_create(self, ctx, n, g, h, u, h_scale, out):
        self.created.append((n, g, h, u, h_scale))
        out._obj.value = 0x1000 + len(self.created)
        return 0

    def bpmi_ipa_batch_prover_destroy(self, handle):
        self.destroyed.append(handle)

    def bpmi_ipa_prove_batch_transcript_bytes(self, handle, protocol, seed_len):
        return 1 + 4 * ((seed_len + 2) // 3) + 80

    def bpmi_ipa_prove_batch(self, *args):
        self.proved.append(args)
        return 0


class StubEngine:
    def __init__(self):
        self.lib, self.ctx = StubLib(), None

    def _ck(self, rc):
        assert rc == 0


def test_constructor_checks_come_before_the_engine():
    eng = StubEngine()
    for g, h, hs in (([], [], None), ([G] * 3, [G] * 3, None), ([G] * 4, [G] * 2, None), ([G] * 4, [G] * 4, [1, 2, 3])):
        with pytest.raises(ValueError, match="power-of-two length"):
            BatchInnerProductProver(g, h, G, h_scale=hs, engine=eng)
    with pytest.raises(ValueError, match="at most 1024 elements.*NIProver / FastNIProver2"):
        BatchInnerProductProver([G] * 2048, [G] * 2048, G, engine=eng)
    assert eng.lib.created == []


def test_constructor_hands_over_packed_generators_and_scale():
    eng = StubEngine()
    g = PackedPoints([G] * 4)
    bp = BatchInnerProductProver(g, [G] * 4, G, h_scale=[0, 1, Q - 1, Q + 5], engine=eng)
    n, gb, hb, ub, sb = eng.lib.created[0]
    assert n == 4 and gb is g.packed and hb == G.to_le64() * 4 and ub == G.to_le64()
    assert sb == b"".join(v.to_bytes(32, "little") for v in (0, 1, Q - 1, 5))
    assert bp.n == 4 and bp.k == 2
    bp.close()
    bp.close()                                                   # idempotent
    assert eng.lib.destroyed == [0x1001]
    BatchInnerProductProver([G], [G], G, engine=eng).close()     # one element: no rounds
    assert eng.lib.created[1][4] is None


def test_prove_checks_come_before_the_native_call():
    eng = StubEngine()
    bp = BatchInnerProductProver([G] * 4, [G] * 4, G, engine=eng)
    a = [[ModP(i + 1, Q) for i in range(4)]] * 3
    short = [[1, 2, 3]] * 3
    with pytest.raises(ValueError, match="every vector of this prover has 4 elements"):
        bp.prove2(short, a)
    with pytest.raises(ValueError, match="every vector of this prover has 4 elements"):
        bp.prove1([G] * 3, [1] * 3, a, short, [b""] * 3)
    with pytest.raises(ValueError, match="same length"):
        bp.prove2(a, a[:2])
    with pytest.raises(ValueError, match="same length"):
        bp.prove1([G] * 2, [1] * 3, a, a, [b""] * 3)
    with pytest.raises(ValueError, match="same length"):
        bp.prove1([G] * 3, [1] * 2, a, a, [b""] * 3)
    with pytest.raises(ValueError, match="one seed per proof"):
        bp.prove1([G] * 3, [1] * 3, a, a, [b"s"] * 2)
    with pytest.raises(ValueError, match="one seed per proof"):
        bp.prove2(a, a, [b"t&"] * 4)
    with pytest.raises(ValueError, match="one seed per proof"):
        bp.prove2_packed(a, a, (b"abc", [0, 1, 2]))
    with pytest.raises(ValueError, match="whole vectors"):
        bp.prove2_packed(bytes(32 * 5), bytes(32 * 5))
    assert eng.lib.proved == []
    assert bp.prove2([], []) == [] and bp.prove1([], [], [], [], []) == []          # an empty batch never reaches the library
    assert eng.lib.proved == []
    bp.close()


def test_what_reaches_the_library():
    """Protocol 2 hands NULL for c, P and head; Protocol 1 without cs hands NULL for c; the seeds arrive joined with their offsets."""
    eng = StubEngine()
    bp = BatchInnerProductProver([G] * 2, [G] * 2, G, engine=eng)
    a = [[1, 2], [3, 4], [Q - 1, 0]]
    bp.prove2_packed(a, a, [b"ab&", None, b"c"])
    args = eng.lib.proved[0]
    assert args[1] == 2 and args[2] == 3 and args[5] is None and args[6] is None and args[12] is None
    assert args[3] == b"".join(v.to_bytes(32, "little") for row in a for v in row)
    assert args[7] == b"ab&c" and list(args[8]) == [0, 3, 3, 4]
    assert isinstance(args[8], ctypes.Array) and args[14] == 3 * eng.lib.bpmi_ipa_prove_batch_transcript_bytes(None, 2, 3)
    bp.prove1_packed([G] * 3, None, a, a, [b"", b"xy", b"z"])
    args = eng.lib.proved[1]
    assert args[1] == 1 and args[5] is None and args[6] == G.to_le64() * 3 and args[12] is not None
    bp.prove1_packed(G.to_le64() * 3, [5, 6, 7], a, a, (b"xyz", [0, 0, 2, 3]))
    args = eng.lib.proved[2]
    assert args[5] == b"".join(v.to_bytes(32, "little") for v in (5, 6, 7)) and list(args[8]) == [0, 0, 2, 3]
    bp.close()
