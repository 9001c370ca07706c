"""Pedersen commitments (reference: src/utils/commitments.py:5-13)."""
from ..ec import Point, pack_points, pack_scalars
from ..pippenger import PipSECP256k1
from .. import engine as _engine


def commitment(g, h, x, r):
    """x*g + r*h -- one 2-term MSM on the GPU instead of two scalar mults and an add."""
    eng = _engine.default_engine()
    return Point.from_le64(eng.msm_bytes(pack_points([g, h]), pack_scalars([x, r]), 2))


def vector_commitment(g, h, a, b):
    assert len(g) == len(h) == len(a) == len(b)
    return PipSECP256k1.multiexp(g + h, a + b)


def vector_commitment_fixed(fx, a, b):
    """vector_commitment(g, h, a, b) over a FixedBasePoints `fx` built once over g + h (pippenger.FixedBasePoints)."""
    assert len(a) == len(b) and len(a) + len(b) == len(fx)
    return PipSECP256k1.multiexp(fx, a + b)


def vector_commitment_batch(g, h, A, B):
    """[vector_commitment(g, h, a, b) for a, b in zip(A, B)] in one native call: the generators are uploaded once and stay two segments
    (g | h) of bpmi_msm_batch_dev, the rows of A and of B are its two scalar matrices -- no list concatenation."""
    A, B = list(A), list(B)
    assert len(A) == len(B)
    for a, b in zip(A, B):
        assert len(g) == len(h) == len(a) == len(b)
    if not A:
        return []
    n = len(g)
    if n == 0:
        return [PipSECP256k1.G.unit for _ in A]
    eng = _engine.default_engine()
    order = PipSECP256k1.order
    bufs = [eng.upload(pack_points(g)), eng.upload(pack_points(h)),
            eng.upload(b"".join(pack_scalars(a, order) for a in A)), eng.upload(b"".join(pack_scalars(b, order) for b in B))]
    try:
        out = eng.msm_batch_dev(bufs[:2], [n, n], bufs[2:], len(A))
    finally:
        for d in bufs:
            d.free()
    return [Point.from_le64(out[64 * v: 64 * v + 64]) for v in range(len(A))]
