"""BatchInnerProductProver.commit / commit_packed -- the statements of a batch from the prover's tables
(bpmi_ipa_batch_prover_commit_batch) -- where they run without a GPU: the argument checks that come before the native call, and what
reaches the library, on a stub engine that records it (src/utils/commitments.py:13 is the function whose loop it replaces)."""
import ctypes

import pytest

import bulletproofs_amd  # noqa: F401
from bulletproofs_amd.ec import Point, secp256k1
from bulletproofs_amd.innerproduct import BatchInnerProductProver
from bulletproofs_amd.utils.utils import ModP

Q = secp256k1.q
G = Point._raw(secp256k1.gx, secp256k1.gy)


class StubLib:
    """create hands out a handle; commit records its arguments and writes G into every slot of the output."""

    def __init__(self):
        self.created, self.destroyed, self.committed = [], [], []

    def bpmi_ipa_batch_prover_create(self, ctx, n, g, h, u, h_scale, out):
        self.created.append((n, g, h, u, h_scale))
        out._obj.value = 0x2000 + len(self.created)
        return 0

    def bpmi_ipa_batch_prover_destroy(self, handle):
        self.destroyed.append(handle)

    def bpmi_ipa_batch_prover_commit_batch(self, handle, count, a, b, u_mode, t, out):
        self.committed.append((handle, count, a, b, u_mode, t))
        ctypes.memmove(out, G.to_le64() * count, 64 * count)
        return 0


class StubEngine:
    def __init__(self):
        self.lib, self.ctx = StubLib(), None

    def _ck(self, rc):
        assert rc == 0


def sc(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


@pytest.fixture
def bp():
    eng = StubEngine()
    prover = BatchInnerProductProver([G] * 4, [G] * 4, G, engine=eng)
    yield prover
    prover.close()


def test_commit_checks_come_before_the_native_call(bp):
    a = [[ModP(i + 1, Q) for i in range(4)]] * 3
    short = [[1, 2, 3]] * 3
    with pytest.raises(ValueError, match="both None"):
        bp.commit(None, None)
    with pytest.raises(ValueError, match="both None"):
        bp.commit_packed(None, None, [1, 2])
    with pytest.raises(ValueError, match="every vector of this prover has 4 elements"):
        bp.commit(short, a)
    with pytest.raises(ValueError, match="every vector of this prover has 4 elements"):
        bp.commit(None, short)
    with pytest.raises(ValueError, match="whole vectors"):
        bp.commit_packed(bytes(32 * 5), None)
    with pytest.raises(ValueError, match="same length"):
        bp.commit(a, a[:2])
    with pytest.raises(ValueError, match="same length"):
        bp.commit_packed(sc(range(8)), sc(range(12)), "inner")
    with pytest.raises(ValueError, match='"inner" sums <a, b>: it takes both'):
        bp.commit(a, None, "inner")
    with pytest.raises(ValueError, match='"inner" sums <a, b>: it takes both'):
        bp.commit(None, a, "inner")
    with pytest.raises(ValueError, match='None, "inner", or one scalar per statement'):
        bp.commit(a, a, "outer")
    with pytest.raises(ValueError, match="one scalar per statement"):
        bp.commit(a, a, [1, 2])
    with pytest.raises(ValueError, match="one scalar per statement"):
        bp.commit(a, None, [1, 2, 3, 4])
    with pytest.raises(ValueError, match="one scalar per statement"):
        bp.commit_packed(a, a, bytes(32 * 3 + 1))
    with pytest.raises(ValueError, match="one scalar per statement"):
        bp.commit(a, a, [])
    assert bp._engine.lib.committed == []
    assert bp.commit([], []) == [] and bp.commit_packed([], None) == b"" and bp.commit([], [], "inner") == []      # an empty batch never reaches the library
    assert bp.commit_packed(b"", b"", b"") == b""
    assert bp._engine.lib.committed == []


def test_what_reaches_the_library(bp):
    """u_term None / "inner" / scalars are u_mode 0 / 1 / 2; a None vector arrives as NULL; t only under u_mode 2, reduced mod q."""
    lib = bp._engine.lib
    a = [[1, 2, 3, 4], [5, 6, 7, Q - 1]]
    b = [[ModP(9, Q)] * 4, [ModP(0, Q)] * 4]
    ab, bb = sc(v for row in a for v in row), sc([9] * 4 + [0] * 4)
    pts = bp.commit(a, b)
    assert lib.committed[-1] == (bp._handle, 2, ab, bb, 0, None)
    assert [p.to_le64() for p in pts] == [G.to_le64()] * 2
    assert bp.commit_packed(ab, bb, "inner") == G.to_le64() * 2
    assert lib.committed[-1] == (bp._handle, 2, ab, bb, 1, None)
    bp.commit(a, b, [Q + 3, 7])
    assert lib.committed[-1] == (bp._handle, 2, ab, bb, 2, sc([3, 7]))
    bp.commit(a, None, sc([0, Q - 1]))
    assert lib.committed[-1] == (bp._handle, 2, ab, None, 2, sc([0, Q - 1]))
    bp.commit_packed(None, bytearray(bb))
    assert lib.committed[-1] == (bp._handle, 2, None, bb, 0, None)
    assert len(lib.committed) == 5
