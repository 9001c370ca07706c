"""Batch verification of inner-product proofs of DIFFERENT lengths over the prefixes of one generator list in ONE multi-scalar
multiplication (bpmi_ipa_verify_batch_mixed_dev; the per-proof verifiers are Verifier1 / Verifier2 of inner_product_verifier.py,
reference: src/innerproduct/inner_product_verifier.py:44-58, :91-102 and :127-147).

A generator list is a capacity: a statement of n_p = 2^k_p elements is made over g[:n_p], h[:n_p] (and h_scale[:n_p]), and its
verifier is Verifier2(g[:n_p], h[:n_p], ...).  Under the random weights of BatchInnerProductVerifier (batch.py: its soundness note
applies unchanged) generator i collects the weighted s-vector entries of the proofs that reach it, so arguments of 64, 256 and 4 096
elements are one MSM of 2 n_top + (extra pairs), n_top the longest length queued, instead of one batch per length plus a sum."""
import secrets

from ..ec import pack_points, pack_scalars
from .batch import CALL_MAX, BatchInnerProductVerifier, Q, _Item, locate_by_bisection
from .inner_product_verifier import Verifier2


class MixedBatchInnerProductVerifier:
    """Verifier2 / Verifier1 for many proofs of different lengths over the prefixes of the same g, h (and the same optional h_scale).

    Which call for which batch (measured: profiles/r16_ipa_verify_mixed.txt).  Proofs of two or more lengths: this
    class -- 1.4-1.5x ahead of one BatchInnerProductVerifier per length plus a sum at 2 .. 16 proofs (add + verify; 1.6-1.9x on verify()
    alone), and level with it, inside the spread, from a few hundred proofs on, where both are the host's re-hash and packing (the device
    then does 0.7 ms of work against 1.7).  No composition was measured at which the per-length loop is ahead.  Proofs of ONE length:
    BatchInnerProductVerifier -- the same plan and the same MSM (ratio 0.99).  PACKED proofs (the arrays of BatchInnerProductProver, one
    prover per length): verify_packed2 / verify_packed1 / locate_packed* below -- one native call over a list of classes."""

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

    # ---- packed proofs of different lengths: a list of classes ---------------------------------------------------------------------
    # A CLASS is the argument tuple of BatchInnerProductVerifier.verify_packed2 / verify_packed1 -- what prove2_packed / prove1_packed of
    # ONE BatchInnerProductProver (one n, over a prefix of this verifier's generators) return, plus the statements.  The whole list is one
    # native call (bpmi_ipa_verify_batch_packed_mixed_dev): every class is re-hashed, checked, inverted and weighted on the device, one
    # launch per round over all classes, then one mixed s-vector sum and ONE MSM.  Nothing is queued.  Proofs are numbered class-major.
    # Measured (profiles/r17_ipa_verify_packed_mixed.txt): 4 096 x 64 + 1 024 x 256 + 256 x 1 024 + 16 x 2^16 in 3.66 ms
    # against 4.93 for one packed call per length plus a sum (1.35x; 2.1x at sixteen proofs of four lengths) and 247 ms for add() + verify()
    # (67x).  ONE length: level with BatchInnerProductVerifier.verify_packed2 (0.81 against 0.80 ms), which stays the call for it.  TWO
    # proofs: add() + verify() wins, 0.39 ms against 0.67 -- the preparation's launches are this path's floor (0.34 ms of device time) --
    # and stays the right path for very few proofs; from sixteen proofs on the packed call is ahead (1.25 ms against 1.64).
    def _packed_classes(self, protocol, classes):
        """Per class: (k, rows, sizes, count).  k is read from the class's rows and checked against lr; a k above the capacity is refused."""
        out = []
        for args in classes:
            if protocol == 2:
                us, Ps, ab, xs, lr, trs = args[:6]
                starts = args[6] if len(args) > 6 else None
                count = len(trs)
                k = packed_class_k(count, xs, lr)
                if k > self.k:
                    raise ValueError("a class of 2^%d elements over a capacity of 2^%d generators" % (k, self.k))
                out.append((k,) + BatchInnerProductVerifier._packed_rows(self, 2, us, Ps, None, ab, xs, lr, None, trs, starts, k))
            else:
                u, Ps, cs, ab, xs, lr, head, trs = args
                count = len(trs)
                k = packed_class_k(count, xs, lr)
                if k > self.k:
                    raise ValueError("a class of 2^%d elements over a capacity of 2^%d generators" % (k, self.k))
                out.append((k,) + BatchInnerProductVerifier._packed_rows(self, 1, u, Ps, cs, ab, xs, lr, head, trs, None, k))
        return out

    def _mixed_calls(self, protocol, prepared, idx, weights):
        """[(out, status)] of the native calls over the proofs idx (sorted global, class-major indices; None: every proof, cut class
        by class without a loop over proofs): consecutive calls cut where a cap of the ABI (2^16 proofs, 2^22 extra pairs, 64 classes)
        would be passed.  weights: packed bytes for exactly idx, or None."""
        pairs = [2 * k + (4 if protocol == 1 else 2) for k, _, _, _ in prepared]
        per = 32 * (3 if protocol == 1 else 1)
        if idx is None:
            calls = [[(c, range(lo, hi)) for c, lo, hi in call] for call in split_mixed_ranges([p[3] for p in prepared], pairs)]
        else:
            owner = []                                     # global index -> (class, local index)
            for c, (_, _, _, count) in enumerate(prepared):
                owner += [(c, i) for i in range(count)]
            calls = []
            for lo, hi in split_mixed_calls([(owner[g][0], pairs[owner[g][0]]) for g in idx]):
                groups = []                                # [(class, [local indices])], class-major
                for g in idx[lo:hi]:
                    c, i = owner[g]
                    if groups and groups[-1][0] == c:
                        groups[-1][1].append(i)
                    else:
                        groups.append((c, [i]))
                calls.append(groups)
        results, at = [], 0
        for groups in calls:
            cls = []
            for c, loc in groups:
                k, rows, sizes, _ = prepared[c]
                if isinstance(loc, range):
                    cut = lambda name: rows[name][sizes[name] * loc.start: sizes[name] * loc.stop]
                    trs = rows["trs"][loc.start: loc.stop]
                    starts = None if rows["starts"] is None else rows["starts"][loc.start: loc.stop]
                else:
                    cut = lambda name: b"".join(rows[name][sizes[name] * i: sizes[name] * (i + 1)] for i in loc)
                    trs = [rows["trs"][i] for i in loc]
                    starts = None if rows["starts"] is None else [rows["starts"][i] for i in loc]
                u = rows["u"] if protocol == 1 else cut("u")
                cls.append((k, len(loc), cut("ab"), cut("xs"), cut("lr"), trs, starts, u, cut("P"), cut("c"), cut("head")))
            count = sum(len(loc) for _, loc in groups)
            seed = None if weights is not None else secrets.token_bytes(32)
            results.append(self.engine.ipa_verify_batch_packed_mixed_dev(self._d[0], self._d[1], self.n, protocol, cls,
                                                                         None if weights is None else weights[per * at: per * (at + count)], seed, self._d_scale))
            at += count
        return results

    def _verify_packed_mixed(self, protocol, classes, weights):
        prepared = self._packed_classes(protocol, classes)
        total = sum(p[3] for p in prepared)
        wb = BatchInnerProductVerifier._weights_bytes(self, protocol, weights, total)
        return all(out == bytes(64) and not any(status) for out, status in self._mixed_calls(protocol, prepared, None, wb))

    def _locate_packed_mixed(self, protocol, classes):
        prepared = self._packed_classes(protocol, classes)
        total = sum(p[3] for p in prepared)
        status = b"".join(st for _, st in self._mixed_calls(protocol, prepared, None, None))
        flagged = [i for i, s in enumerate(status) if s]
        rest = [i for i, s in enumerate(status) if not s]

        def probe(sub):
            return all(out == bytes(64) and not any(st) for out, st in self._mixed_calls(protocol, prepared, [rest[j] for j in sub], None))
        return sorted(flagged + [rest[j] for j in locate_by_bisection(len(rest), probe)])

    def verify_packed2(self, classes, weights=None):
        """True iff every Protocol-2 proof of every class is valid for its statement over the prefix of its own length.  classes: a list
        of the argument tuples of BatchInnerProductVerifier.verify_packed2 -- (us, Ps, ab, xs, lr, transcripts[, starts]) -- one per
        length (or several of one length), in any order; a class's k is read from its rows.  Random weights come from a fresh 32-byte
        seed per native call; weights: one integer per proof, class-major, instead (tests).  A batch beyond 2^16 proofs, 2^22 extra pairs
        or 64 classes runs as consecutive calls.

        Which call for which batch (measured: profiles/r17_ipa_verify_packed_mixed.txt): two or more lengths and
        more than a handful of proofs -- this call (1.35-2.1x ahead of one packed call per length plus a sum, 67-99x ahead of add() +
        verify() from a few thousand proofs on).  ONE length: BatchInnerProductVerifier.verify_packed2, the same work (0.80 against 0.81
        ms).  Very few proofs: the object path, add() + verify(), stays the right one -- 0.39 ms against 0.67 at two proofs of two lengths,
        because the preparation's launches are this call's floor; at sixteen proofs this call is ahead (1.25 against 1.64 ms)."""
        return self._verify_packed_mixed(2, classes, weights)

    def verify_packed1(self, classes, weights=None):
        """verify_packed2 for Protocol-1 classes: tuples (u, Ps, cs, ab, xs, lr, head, transcripts) as BatchInnerProductVerifier.verify_packed1
        takes them; weights: three integers (w, r1, r2) per proof, class-major, instead of the random ones (tests)."""
        return self._verify_packed_mixed(1, classes, weights)

    def locate_packed2(self, classes):
        """The sorted GLOBAL (class-major) indices of the invalid proofs of a list of packed Protocol-2 classes: those the status bytes
        flag, and the rest found by locate_by_bisection, every probe one mixed native call over the gathered rows of the subset."""
        return self._locate_packed_mixed(2, classes)

    def locate_packed1(self, classes):
        """locate_packed2 for Protocol-1 classes."""
        return self._locate_packed_mixed(1, classes)


PAIRS_MAX = 1 << 22            # extra pairs per native call (IPAB_EXTRA_MAX)
CLASSES_MAX = 64               # classes per native call (IPAPM_CLASSES_MAX)


def packed_class_k(count, xs, lr):
    """The round count of a packed class read from its rows: len(xs) // (32 count), checked against lr (k = 0: both empty)."""
    if count == 0:
        if len(xs) or len(lr):
            raise ValueError("an empty class has no rows")
        return 0
    k = len(xs) // (32 * count)
    if len(xs) != 32 * k * count or len(lr) != 128 * k * count:
        raise ValueError("xs: k x 32 bytes and lr: 2k x 64 bytes per proof, one row per transcript")
    return k


def split_mixed_calls(items, proofs_max=CALL_MAX, pairs_max=PAIRS_MAX, classes_max=CLASSES_MAX):
    """items: per proof, class-major, (class, extra pairs of the proof).  The slices [(lo, hi)] of consecutive native calls: each as
    long as the caps allow."""
    cuts, lo, pairs, classes, last = [], 0, 0, 0, None
    for i, (c, pp) in enumerate(items):
        new_class = 1 if c != last else 0
        if i > lo and (i - lo == proofs_max or pairs + pp > pairs_max or classes + new_class > classes_max):
            cuts.append((lo, i))
            lo, pairs, classes, new_class = i, 0, 0, 1
        pairs, classes, last = pairs + pp, classes + new_class, c
    if len(items) > lo:
        cuts.append((lo, len(items)))
    return cuts


def split_mixed_ranges(counts, pairs, proofs_max=CALL_MAX, pairs_max=PAIRS_MAX, classes_max=CLASSES_MAX):
    """split_mixed_calls for EVERY proof of classes of counts[c] proofs with pairs[c] extra pairs each, without a loop over proofs: per
    native call the list of (class, lo, hi) row ranges, class-major; the same cuts."""
    calls, cur, n, pr = [], [], 0, 0
    for c, (count, pp) in enumerate(zip(counts, pairs)):
        lo = 0
        while lo < count:
            if cur and (len(cur) == classes_max or n == proofs_max or pr + pp > pairs_max):
                calls.append(cur)
                cur, n, pr = [], 0, 0
            take = max(1, min(count - lo, proofs_max - n, (pairs_max - pr) // pp))
            cur.append((c, lo, lo + take))
            n, pr, lo = n + take, pr + take * pp, lo + take
    if cur:
        calls.append(cur)
    return calls


def batch_verify_inner_products_mixed(g, h, statements, h_scale=None, engine=None, rng=None):
    """True iff every (u, P, proof2) of `statements` is a valid Protocol-2 proof over the prefix of g, h of its own length."""
    bv = MixedBatchInnerProductVerifier(g, h, h_scale, engine, rng)
    try:
        for u, P, proof2 in statements:
            bv.add(u, P, proof2)
        return bv.verify()
    finally:
        bv.release()
