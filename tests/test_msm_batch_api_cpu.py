"""The Python surface of the batched MSM -- Pippenger.multiexp_batch, vector_commitment_batch -- where it runs without a GPU: the
argument checks that come before the engine is touched, and the loop over multiexp that any group other than secp256k1 gets, on the
counting group of tests/golden/modp_group.json (src/pippenger/pippenger.py:22-61 is what each row computes)."""
import pytest

import bulletproofs_amd  # noqa: F401
from bulletproofs_amd import engine as engine_mod
from bulletproofs_amd.ec import Point, secp256k1
from bulletproofs_amd.pippenger import PipSECP256k1
from bulletproofs_amd.pippenger.group import MultIntModP
from bulletproofs_amd.pippenger.modp import ModP
from bulletproofs_amd.pippenger.pippenger import Pippenger
from bulletproofs_amd.utils import vector_commitment_batch
from bulletproofs_amd.utils.commitments import vector_commitment_batch as from_module

from conftest import load_golden


@pytest.fixture
def no_engine(monkeypatch):
    """Any use of the engine fails the test: these paths must return or raise before it."""
    def boom():
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(engine_mod, "default_engine", boom)


def test_multiexp_batch_checks_come_before_the_engine(no_engine):
    G = Point._raw(secp256k1.gx, secp256k1.gy)
    with pytest.raises(Exception, match="Different number of group elements and exponents"):
        PipSECP256k1.multiexp_batch([G, G], [[1, 2], [3]])                 # a ragged row: multiexp's own exception
    with pytest.raises(Exception, match="Different number of group elements and exponents"):
        PipSECP256k1.multiexp_batch([G], [[1], [2], []])
    with pytest.raises(Exception, match="Different number of group elements and exponents"):
        PipSECP256k1.multiexp_batch([], [[], [7]])
    assert PipSECP256k1.multiexp_batch([G, G], []) == []
    assert PipSECP256k1.multiexp_batch([], []) == []
    units = PipSECP256k1.multiexp_batch([], [[], [], []])                   # no bases: the unit once per row
    assert units == [PipSECP256k1.G.unit] * 3
    assert PipSECP256k1.multiexp_batch([G], iter([])) == []                 # any iterable of rows


def test_vector_commitment_batch_checks_come_before_the_engine(no_engine):
    assert vector_commitment_batch is from_module
    G = Point._raw(secp256k1.gx, secp256k1.gy)
    assert vector_commitment_batch([G], [G], [], []) == []
    with pytest.raises(AssertionError):
        vector_commitment_batch([G], [G], [[1], [2]], [[3]])                # A and B of different lengths
    with pytest.raises(AssertionError):
        vector_commitment_batch([G], [G, G], [[1]], [[3]])                  # g and h
    with pytest.raises(AssertionError):
        vector_commitment_batch([G, G], [G, G], [[1, 2], [1]], [[3, 4], [5, 6]])       # a ragged row
    assert vector_commitment_batch([], [], [[], []], [[], []]) == [PipSECP256k1.G.unit] * 2


def test_multiexp_batch_on_another_group_is_the_loop(no_engine):
    for c in load_golden("modp_group.json")["cases"]:
        p, n = c["p"], c["n"]
        pip = Pippenger(MultIntModP(p, p - 1))
        gs = [ModP(2 + 3 * i, p) for i in range(n)]                  # same inputs as tests/golden/make_golden.py
        rows = [[(12345 * (i + 1) ** 3) % (p - 1) for i in range(n)],
                [(7 * i + 1) % (p - 1) for i in range(n)], [0] * n, [p - 1 + 5 + i for i in range(n)], [-3 - i for i in range(n)]]
        ModP.reset()
        want = [pip.multiexp(gs, r) for r in rows]
        loop_mults = ModP.num_of_mult
        ModP.reset()
        got = pip.multiexp_batch(gs, rows)
        assert [g.x for g in got] == [w.x for w in want] and got[0].x == c["result"]
        assert ModP.num_of_mult == loop_mults                        # the loop, multiplication for multiplication
        assert got[2].x == 1
        with pytest.raises(Exception, match="Different number of group elements and exponents"):
            pip.multiexp_batch(gs, rows + [[1] * (n + 1)])
        assert pip.multiexp_batch(gs, []) == []
    pip = Pippenger(MultIntModP(101, 100))
    assert pip.multiexp_batch([], [[], []]) == [ModP(1, 101)] * 2
