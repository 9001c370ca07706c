"""Batch verification of inner-product proofs of DIFFERENT lengths over the prefixes of one generator list in ONE multi-scalar
multiplication (bpmi_ipa_verify_batch_mixed_dev; the per-proof verifiers are Verifier1 / Verifier2 of inner_product_verifier.py,
reference: src/innerproduct/inner_product_verifier.py:44-58, :91-102 and :127-147).

A generator list is a capacity: a statement of n_p = 2^k_p elements is made over g[:n_p], h[:n_p] (and h_scale[:n_p]), and its
verifier is Verifier2(g[:n_p], h[:n_p], ...).  Under the random weights of BatchInnerProductVerifier (batch.py: its soundness note
applies unchanged) generator i collects the weighted s-vector entries of the proofs that reach it, so arguments of 64, 256 and 4 096
elements are one MSM of 2 n_top + (extra pairs), n_top the longest length queued, instead of one batch per length plus a sum."""
from ..ec import pack_points, pack_scalars
from .batch import BatchInnerProductVerifier, Q, _Item
from .inner_product_verifier import Verifier2


class MixedBatchInnerProductVerifier:
    """Verifier2 / Verifier1 for many proofs of different lengths over the prefixes of the same g, h (and the same optional h_scale).

    Which call for which batch (measured: profiles/r16_ipa_verify_mixed.txt).  Proofs of two or more lengths: this
    class -- 1.4-1.5x ahead of one BatchInnerProductVerifier per length plus a sum at 2 .. 16 proofs (add + verify; 1.6-1.9x on verify()
    alone), and level with it, inside the spread, from a few hundred proofs on, where both are the host's re-hash and packing (the device
    then does 0.7 ms of work against 1.7).  No composition was measured at which the per-length loop is ahead.  Proofs of ONE length:
    BatchInnerProductVerifier -- the same plan and the same MSM (ratio 0.99), and it has the packed path, which this class has not."""

    def __init__(self, g, h, h_scale=None, engine=None, rng=None):
        """g, h: the capacity lists, 2^K points each (lists of points or PackedPoints), uploaded once; h_scale: 2^K integers c_i or
        None; rng() -> int: the source of the random weights (default: secrets).  As BatchInnerProductVerifier."""
        BatchInnerProductVerifier.__init__(self, g, h, h_scale, engine, rng)

    __len__ = BatchInnerProductVerifier.__len__
    reset = BatchInnerProductVerifier.reset
    release = BatchInnerProductVerifier.release
    _weight = BatchInnerProductVerifier._weight
    add_proof1 = BatchInnerProductVerifier.add_proof1
    verify = BatchInnerProductVerifier.verify
    locate = BatchInnerProductVerifier.locate

    def _queue2(self, u, P, proof2, head=()):
        it = _Item()
        self._items.append(it)
        try:
            k = len(proof2.Ls)                         # the proof's own round count: its statement is over g[:2^k], h[:2^k]
            if k > self.k or len(proof2.Rs) != k or len(proof2.xs) != k:
                raise ValueError("a proof longer than the capacity, or one whose lists disagree")
            v = Verifier2(None, None, u, P, proof2)
            v.verify_transcript(k)
            xv, xi, pts, scs = v._extra_terms()        # refuses a challenge = 0 (mod q)
            it.xs, it.xinvs = [x % Q for x in xv], [x % Q for x in xi]
            it.a, it.b = proof2.a.x % Q, proof2.b.x % Q
            it.groups = ((list(pts), [int(s) % Q for s in scs]),) + tuple(head)
            for pts_g, _ in it.groups:
                for p in pts_g:
                    p.to_le64()
            it.valid = True
        except Exception:
            it.valid = False                           # "Proof invalid" at the byte level: it never reaches the device
        return len(self._items) - 1

    def add(self, u, P, proof2):
        """Queue a Protocol-2 proof of the statement (u, P); returns its index.  Its length 2^k is its own round count, k = len(proof2.Ls);
        a proof of more rounds than the capacity has is recorded as invalid.  The transcript is re-derived here, on the host
        (Verifier2.verify_transcript(k))."""
        return self._queue2(u, P, proof2)

    def _probe(self, idx, weights):
        """True iff the weighted sum of the equations of the (host-valid) proofs idx is the identity: one native call over all their
        lengths."""
        ks, xs, xinvs, a, b, pts, scs = [], [], [], [], [], [], []
        for i, w in zip(idx, weights):
            it = self._items[i]
            ks.append(len(it.xs))
            xs += it.xs
            xinvs += it.xinvs
            a.append(it.a)
            b.append(it.b)
            for gi, (gp, gs) in enumerate(it.groups):
                r = w if gi == 0 else self._weight()
                pts += gp
                scs += [s * r % Q for s in gs]
        out = self.engine.ipa_verify_batch_mixed_dev(self._d[0], self._d[1], self.n, ks, pack_scalars(xs, Q), pack_scalars(xinvs, Q), pack_scalars(a, Q),
                                                     pack_scalars(b, Q), pack_scalars([w % Q for w in weights], Q), pack_points(pts),
                                                     pack_scalars(scs, Q), len(pts), self._d_scale)
        return out == bytes(64)


def batch_verify_inner_products_mixed(g, h, statements, h_scale=None, engine=None, rng=None):
    """True iff every (u, P, proof2) of `statements` is a valid Protocol-2 proof over the prefix of g, h of its own length."""
    bv = MixedBatchInnerProductVerifier(g, h, h_scale, engine, rng)
    try:
        for u, P, proof2 in statements:
            bv.add(u, P, proof2)
        return bv.verify()
    finally:
        bv.release()
