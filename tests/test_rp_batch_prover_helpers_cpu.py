"""What BatchRangeProver and MixedBatchRangeProver share on the Python side (rangeproofs/batch_prover.py: pack_scalars, pack_pairs,
seed_offsets, grown_output), where it runs without a GPU: the three input forms give the same bytes, the argument errors keep their
texts, and the page-locked output buffer grows by the provers' rule on a stub engine."""
import ctypes

import pytest

import bulletproofs_amd  # noqa: F401
from bulletproofs_amd.ec import secp256k1
from bulletproofs_amd.rangeproofs.batch_prover import grown_output, pack_pairs, pack_scalars, seed_offsets
from bulletproofs_amd.utils.utils import ModP

Q = secp256k1.q


def le(vals):
    return b"".join((v % Q).to_bytes(32, "little") for v in vals)


def test_the_three_input_forms_give_the_same_bytes():
    vals = [0, 1, Q - 1, Q + 5, 1 << 200, 7]
    want = le(vals)
    assert pack_scalars(vals, 1) == pack_scalars([ModP(v, Q) for v in vals], 1) == want                  # flat: proofs of one value
    assert pack_scalars([[v] for v in vals], 1) == want                                                   # rows of one
    for m in (2, 3):
        rows = [vals[i: i + m] for i in range(0, len(vals), m)]
        assert pack_scalars(rows, m) == pack_scalars([tuple(r) for r in rows], m) == want                 # rows of m
        assert pack_scalars(want, m) == pack_scalars(bytearray(want), m) == pack_scalars(memoryview(want), m) == want      # packed bytes
        assert pack_pairs(rows, want, m) == (want, want, len(vals) // m)
    assert pack_scalars([[1], [2, 3], []]) == le([1, 2, 3]) and pack_scalars([4, 5]) == le([4, 5])       # m=None: rows of any length
    assert pack_scalars([], 4) == b"" and pack_pairs([], b"", 4) == (b"", b"", 0)


@pytest.mark.parametrize("what", ["prover", "class"])
def test_rows_of_the_wrong_length_keep_their_text(what):
    with pytest.raises(ValueError, match="every proof of this %s takes 4 values" % what):
        pack_scalars([[1, 2, 3, 4], [1, 2, 3]], 4, what)
    with pytest.raises(ValueError, match="every proof of this %s takes 4 values" % what):
        pack_scalars([1, 2, 3, 4], 4, what)                          # a flat list for proofs of several values
    with pytest.raises(ValueError, match="every proof of this %s takes 1 values" % what):
        pack_scalars([[1, 2]], 1, what)
    with pytest.raises(ValueError, match="every proof of this %s takes 2 values" % what):
        pack_pairs([[1, 2]], [[1]], 2, what)


def test_values_and_blinding_factors_must_match():
    for vs, gs, m in (([1, 2], [1], 1), ([[1, 2]], [[1, 2], [3, 4]], 2), (bytes(64), bytes(32), 1), (bytes(96), bytes(96), 2), (bytes(33), bytes(33), 1)):
        with pytest.raises(ValueError, match="values and blinding factors must have the same length"):
            pack_pairs(vs, gs, m)


def test_offsets_from_a_list_and_from_bytes_with_offsets_agree():
    seeds = [b"", b"a", b"x" * 100, b"", b"yz"]
    sb, off = seed_offsets(seeds, 5)
    assert sb == b"".join(seeds) and isinstance(off, ctypes.Array) and off._type_ is ctypes.c_uint64
    assert list(off) == [0, 0, 1, 101, 101, 103]
    sb2, off2 = seed_offsets((bytearray(sb), list(off)), 5)
    assert sb2 == sb and isinstance(sb2, bytes) and isinstance(off2, ctypes.Array) and list(off2) == list(off)
    assert seed_offsets((sb, off), 5)[1] is off                      # a ctypes array is taken as it is
    assert seed_offsets([], 0)[0] == b"" and list(seed_offsets([], 0)[1]) == [0]
    for bad in (seeds[:4], (sb, [0, 1, 2]), (sb, list(off) + [103])):
        with pytest.raises(ValueError, match="values, blinding factors and seeds must have the same length"):
            seed_offsets(bad, 5)


class StubBuffer:
    def __init__(self, size):
        self.size, self.freed = size, False

    def __len__(self):
        return self.size

    def free(self):
        self.freed = True


class StubEngine:
    def __init__(self):
        self.allocated = []

    def host_alloc(self, size):
        self.allocated.append(size)
        return StubBuffer(size)


def test_the_output_buffer_grows_with_an_eighth_to_spare_and_is_kept():
    eng = StubEngine()
    a = grown_output(eng, None, 800)
    assert len(a) == 900 and eng.allocated == [900]
    assert grown_output(eng, a, 900) is a and grown_output(eng, a, 16) is a and not a.freed
    b = grown_output(eng, a, 901)
    assert b is not a and a.freed and len(b) == 901 + 901 // 8 and eng.allocated == [900, 1013]
