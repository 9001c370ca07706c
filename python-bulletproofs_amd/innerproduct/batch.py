"""Batch verification of inner-product proofs over shared generators in ONE multi-scalar multiplication
(bpmi_ipa_verify_batch_dev; the per-proof verifiers are Verifier1 / Verifier2 of inner_product_verifier.py,
reference: src/innerproduct/inner_product_verifier.py:44-58 and :127-147).

Verifier2's check is one point equation per proof.  Multiplied by a random weight each and added up, the generator terms of
all proofs collapse to 2n pairs -- their scalars are sums of weighted s-vectors, computed on the device -- so B proofs cost
one MSM of 2n + B (2 log n + 2) pairs instead of B MSMs of 2n.  The weights MUST be unpredictable to whoever made the
proofs: two invalid proofs whose errors are e and -e pass `verify(weights=[1, 1])`, and with any known weights a pair of
errors can be scaled to cancel.  `verify()` draws them from `secrets`.

Two ways in.  Proof OBJECTS: `add` / `add_proof1` re-derive each transcript in Python and `verify()` runs the MSM.  PACKED proofs --
the arrays BatchInnerProductProver.prove2_packed / prove1_packed return: `verify_packed2` / `verify_packed1` hand them to ONE native
call (bpmi_ipa_verify_batch_packed_dev) that re-hashes, compares, inverts and weights every proof on the device, one lane per proof,
and runs the same MSM; the weights come from a fresh 32-byte seed per call, and the note above applies unchanged."""
import ctypes
import math
import secrets

from .. import engine as _engine
from ..ec import PackedPoints, pack_points, pack_scalars, secp256k1
from ..locate import locate_by_bisection, locate_plan        # noqa: F401  (locate_by_bisection: also this module's old export)
from ..utils.utils import mod_hash
from .codec import _split as split_blobs
from .inner_product_verifier import Verifier2

Q = secp256k1.q
CALL_MAX = 1 << 16             # proofs per native call (IPAB_PROOFS_MAX, csrc/ipa_batch_plan_host.hpp)
GROUP_MAX_PAIRS = 8448         # MID_NMAX (csrc/shared_defs.hpp): the pairs of one group's MSM in the one-launch group kernel
GROUP_ROWS_MAX = 1 << 26       # group scalars per native call: groups x 2 n (IPAG_ROWS_MAX, csrc/ipa_group_plan_host.hpp)


def extra_pairs(protocol, k):
    """The extra pairs a packed proof of 2^k elements brings to the MSM (ipap_pairs, csrc/ipa_packed_plan_host.hpp)."""
    return 2 * k + (4 if protocol == 1 else 2)


def weight_bytes(protocol):
    """The bytes of a proof's explicit weights: one scalar under Protocol 2, three (w, r1, r2) under Protocol 1."""
    return 32 * (3 if protocol == 1 else 1)


def default_group_for(protocol, k, count=None):
    """The two rules of default_group / default_groups for `count` packed proofs of 2^k elements."""
    fit = (GROUP_MAX_PAIRS - 2 * (1 << k)) // extra_pairs(protocol, k)
    if fit >= 1:
        return 1 << (fit.bit_length() - 1)
    root = math.isqrt(count) if count and count > 0 else 1
    return 1 << (max(root, 1).bit_length() - 1)


def packed_rows_cut(protocol, rows, sizes, idx):
    """(ab, xs, lr, trs, starts, u, P, c, head) of the rows idx of one packed class (rows, sizes: what _packed_rows returns) -- the
    per-class arguments of the packed native calls, in their order.  idx: a range of step 1 (sliced) or a sorted list (gathered): the
    same bytes either way.  starts stays None where the class has none; under Protocol 1 u is the class's ONE shared point."""
    if isinstance(idx, range) and idx.step == 1:
        cut = lambda name: rows[name][sizes[name] * idx.start: sizes[name] * idx.stop]
        pick = lambda lst: lst[idx.start: idx.stop]
    else:
        cut = lambda name: b"".join(rows[name][sizes[name] * i: sizes[name] * (i + 1)] for i in idx)
        pick = lambda lst: [lst[i] for i in idx]
    return (cut("ab"), cut("xs"), cut("lr"), pick(rows["trs"]), None if rows["starts"] is None else pick(rows["starts"]),
            rows["u"] if protocol == 1 else cut("u"), cut("P"), cut("c"), cut("head"))


class _Item:
    """One queued proof: the inputs of its row of the s-vector sum and its extra pairs, grouped by the weight they take --
    group 0 under the proof's own weight, every further group (the equalities of Protocol 1) under a fresh one."""
    __slots__ = ("valid", "xs", "xinvs", "a", "b", "groups")

    def __init__(self):
        self.valid, self.xs, self.xinvs, self.a, self.b, self.groups = False, (), (), 0, 0, ()


class BatchInnerProductVerifier:
    """Verifier2 / Verifier1 for many proofs over the same generators g, h (and the same optional h_scale)."""

    def __init__(self, g, h, h_scale=None, engine=None, rng=None):
        """g, h: lists of points or PackedPoints (those keep their device copy), n = 2^k each, uploaded once.  h_scale: integers
        c_i, the statements are over c_i * h[i] (see Verifier2), uploaded once.  rng() -> int: the source of the random weights;
        default: secrets (a CSPRNG)."""
        n = len(g)
        if n < 1 or n & (n - 1) or len(h) != n or (h_scale is not None and len(h_scale) != n):
            raise ValueError("g, h (and h_scale) must have the same power-of-two length")
        self.n, self.k = n, n.bit_length() - 1
        self.engine = engine or _engine.default_engine()
        self._rng = rng or (lambda: secrets.randbelow(Q - 1) + 1)
        self._own = []
        self._d = []
        for lst in (g, h):
            if isinstance(lst, PackedPoints):
                self._d.append(lst.device(self.engine))
            else:
                self._d.append(self.engine.upload(pack_points(lst)))
                self._own.append(self._d[-1])
        self._d_scale = None
        if h_scale is not None:
            self._d_scale = self.engine.upload(pack_scalars(h_scale, Q))
            self._own.append(self._d_scale)
        self._keep = (g, h)                      # PackedPoints free their device copy when collected
        self._items = []

    def __len__(self):
        return len(self._items)

    def reset(self):
        """Forget the queued proofs; the generators stay resident."""
        self._items = []

    def release(self):
        """Free the device buffers this object uploaded (not the device copies of PackedPoints)."""
        for d in self._own:
            d.free()
        self._own, self._d, self._d_scale, self._items = [], [], None, []

    def _weight(self):
        return self._rng() % Q or 1

    # ---- queueing ------------------------------------------------------------------------------------------------------------
    def _queue2(self, u, P, proof2, head=()):
        it = _Item()
        self._items.append(it)
        try:
            v = Verifier2(None, None, u, P, proof2)
            v.verify_transcript(self.k)
            xv, xi, pts, scs = v._extra_terms()            # refuses a challenge = 0 (mod q)
            it.xs, it.xinvs = [x % Q for x in xv[:self.k]], [x % Q for x in xi[:self.k]]
            it.a, it.b = proof2.a.x % Q, proof2.b.x % Q
            it.groups = ((list(pts), [int(s) % Q for s in scs]),) + tuple(head)
            for pts_g, _ in it.groups:
                for p in pts_g:
                    p.to_le64()
            it.valid = True
        except Exception:
            it.valid = False                             # "Proof invalid" at the byte level: it never reaches the device
        return len(self._items) - 1

    def add(self, u, P, proof2):
        """Queue a Protocol-2 proof of the statement (u, P); returns its index.  The transcript is re-derived here, on the host
        (Verifier2.verify_transcript); a proof that fails it is recorded as invalid."""
        return self._queue2(u, P, proof2)

    def add_proof1(self, u, P, c, proof1):
        """Queue a Protocol-1 proof of (u, P, c).  Verifier1's re-hash runs on the host; its two equalities P_new = P + x c u and
        u_new = x u join the MSM as five extra pairs, each equality under a random weight of its own."""
        try:
            items = proof1.transcript.split(b"&")
            if items[1] != str(mod_hash(b"&".join(items[:1]) + b"&", Q)).encode():
                raise ValueError("transcript")
            x = int(items[1]) % Q
            cv = (c.x if hasattr(c, "x") else int(c)) % Q
            head = (([proof1.P_new, P, u], [1, Q - 1, (Q - x * cv % Q) % Q]), ([proof1.u_new, u], [1, (Q - x) % Q]))
        except Exception:
            it = _Item()
            self._items.append(it)
            return len(self._items) - 1
        return self._queue2(proof1.u_new, proof1.P_new, proof1.proof2, head)

    # ---- verification --------------------------------------------------------------------------------------------------------
    def _probe(self, idx, weights):
        """True iff the weighted sum of the equations of the (host-valid) proofs idx is the identity: one native call (its per-call
        caps -- include/bpmi.h -- are the engine's to refuse)."""
        xs, xinvs, a, b, pts, scs = [], [], [], [], [], []
        for i, w in zip(idx, weights):
            it = self._items[i]
            xs += it.xs
            xinvs += it.xinvs
            a.append(it.a)
            b.append(it.b)
            for gi, (gp, gs) in enumerate(it.groups):
                r = w if gi == 0 else self._weight()
                pts += gp
                scs += [s * r % Q for s in gs]
        out = self.engine.ipa_verify_batch_dev(self._d[0], self._d[1], self.n, len(idx), pack_scalars(xs, Q), pack_scalars(xinvs, Q),
                                               pack_scalars(a, Q), pack_scalars(b, Q), pack_scalars([w % Q for w in weights], Q),
                                               pack_points(pts), pack_scalars(scs, Q), len(pts), self._d_scale)
        return out == bytes(64)

    def verify(self, weights=None):
        """True iff every queued proof is valid (an empty batch is).  weights: one integer per queued proof instead of the random
        ones -- for tests and for callers that shard a batch under weights drawn elsewhere; never values a prover could know."""
        if weights is not None and len(weights) != len(self._items):
            raise ValueError("one weight per queued proof")
        if not self._items:
            return True
        if not all(it.valid for it in self._items):
            return False
        ws = [int(w) % Q for w in weights] if weights is not None else [self._weight() for _ in self._items]
        return self._probe(list(range(len(self._items))), ws)

    def locate(self):
        """The sorted indices of the invalid proofs: those that failed on the host, and those found by bisection over subsets of the
        rest -- every probe one native call over the resident generators, under fresh weights."""
        good = [i for i, it in enumerate(self._items) if it.valid]
        bad = [i for i, it in enumerate(self._items) if not it.valid]
        found = locate_by_bisection(len(good), lambda sub: self._probe([good[j] for j in sub], [self._weight() for _ in sub]))
        return sorted(bad + [good[j] for j in found])


    # ---- packed proofs: what BatchInnerProductProver.prove2_packed / prove1_packed return ---------------------------------------
    # The whole verification is native (bpmi_ipa_verify_batch_packed_dev; csrc/ipa_packed_kernels.hpp): the transcripts are re-hashed,
    # the items compared, the challenges inverted and the weighted scalars formed on the device, one lane per proof, and the batch
    # is the same one MSM.  Nothing is queued: a call verifies what it is given.  Measured (profiles/r12_ipa_verify_packed.txt): 36-60x
    # faster than add() + verify() over 1 024 proofs of 64 .. 1 024 elements, 2.1x at 16 proofs of 64; SLOWER at one proof (0.39 ms
    # against 0.22) and at three proofs of 4 elements (0.31 against 0.24): three launches of single-wave chains and the uploads are
    # its floor, so add() + verify() stays the right path below a handful of proofs.
    def _packed_rows(self, protocol, u, Ps, cs, ab, xs, lr, head, transcripts, starts, k=None):
        """k: the rows' round count (None: this verifier's; MixedBatchInnerProductVerifier passes a class's own)."""
        to_bytes = lambda v: bytes(v) if isinstance(v, (bytes, bytearray, memoryview)) else pack_points(v)
        count = len(transcripts)
        rows = {"ab": bytes(ab), "xs": bytes(xs), "lr": bytes(lr), "P": to_bytes(Ps), "trs": list(transcripts),
                "starts": None if starts is None else [int(s) for s in starts]}
        if protocol == 1:
            rows["u"] = u if isinstance(u, (bytes, bytearray)) else u.to_le64()
            rows["c"] = bytes(cs) if isinstance(cs, (bytes, bytearray, memoryview)) else pack_scalars(cs, Q)
            rows["head"] = bytes(head)
        else:
            rows["u"], rows["c"], rows["head"] = to_bytes(u), b"", b""
        k = self.k if k is None else k
        sizes = {"ab": 64, "xs": 32 * k, "lr": 128 * k, "P": 64, "c": 32 if protocol == 1 else 0, "head": 128 if protocol == 1 else 0}
        if protocol == 2:
            sizes["u"] = 64
        for name, per in sizes.items():
            if len(rows[name]) != per * count:
                raise ValueError("%s: %d bytes per proof, one row per transcript" % (name, per))
        if (protocol == 1 and len(rows["u"]) != 64) or (rows["starts"] is not None and len(rows["starts"]) != count):
            raise ValueError("u is one point under Protocol 1; one start per proof")
        return rows, sizes, count

    def _packed_call(self, protocol, rows, sizes, idx, weights):
        """(out, status) of one native call over the rows idx (a range or a sorted list; at most 2^16)."""
        seed = None if weights is not None else secrets.token_bytes(32)
        return self.engine.ipa_verify_batch_packed_dev(self._d[0], self._d[1], self.n, protocol, len(idx), *packed_rows_cut(protocol, rows, sizes, idx),
                                                       weights, seed, self._d_scale)

    def _weights_bytes(self, protocol, weights, count):
        if weights is None:
            return None
        flat = [int(w) % Q for row in weights for w in (row if isinstance(row, (tuple, list)) else (row,))]
        if len(flat) != weight_bytes(protocol) // 32 * count:
            raise ValueError("one weight per proof under Protocol 2, three (w, r1, r2) under Protocol 1")
        return pack_scalars(flat, Q)

    def _verify_packed(self, protocol, rows, sizes, count, weights):
        per = weight_bytes(protocol)
        wb = self._weights_bytes(protocol, weights, count)
        for lo in range(0, count, CALL_MAX):               # consecutive calls of at most 2^16 proofs; valid iff every call is
            hi = min(lo + CALL_MAX, count)
            out, status = self._packed_call(protocol, rows, sizes, range(lo, hi), None if wb is None else wb[per * lo: per * hi])
            if out != bytes(64) or status != bytes(hi - lo):
                return False
        return True

    def _locate_packed(self, protocol, rows, sizes, count, group=None):
        if group is None or int(group) >= 1:
            grp = self.default_group(protocol, count) if group is None else int(group)
            return locate_plan(count, grp, lambda idx, g: self._group_values_packed(protocol, rows, sizes, range(count) if idx is None else idx, g, None))
        if int(group) != 0:
            raise ValueError("group must be None, 0 (bisection) or at least 1")
        flagged = []
        for lo in range(0, count, CALL_MAX):
            hi = min(lo + CALL_MAX, count)
            _, status = self._packed_call(protocol, rows, sizes, range(lo, hi), None)
            flagged += [lo + i for i, s in enumerate(status) if s]
        marked = set(flagged)
        rest = [i for i in range(count) if i not in marked]

        def probe(sub):
            for lo in range(0, len(sub), CALL_MAX):
                out, status = self._packed_call(protocol, rows, sizes, [rest[j] for j in sub[lo: lo + CALL_MAX]], None)
                if out != bytes(64) or any(status):
                    return False
            return True
        return sorted(flagged + [rest[j] for j in locate_by_bisection(len(rest), probe)])

    # ---- packed proofs, per GROUP of consecutive proofs: one native call names the groups that hold an invalid proof ---------------
    # bpmi_ipa_group_values_packed_dev (csrc/ipa_group_dev_host.hpp): the preparation of the packed verifier once, the s-vector sums per
    # group, the groups' MSMs over [g | h | the group's extra pairs] in one launch.  locate_packed* is two such calls (locate_plan).
    def default_group(self, protocol, count=None):
        """The group size locate_packed1 / locate_packed2 start with.  Where a group's MSM fits the one-launch group kernel: the largest
        power of two with 2 n + group * per <= 8448 pairs (MID_NMAX, csrc/shared_defs.hpp), per = 2 log2 n + 2 extra pairs of a proof under
        Protocol 2 and 2 log2 n + 4 under Protocol 1.  Where not even one proof fits (n >= 8192) every group is a multi-scalar
        multiplication of its own, and the plan runs count / group + bad * group of them: the largest power of two <= sqrt(count) (1
        without a count).  Both are CAPACITY rules -- what fits a launch, what balances the two levels -- and NOT measured optima:
        profiles/r18_ipa_locate_packed.txt has the first rule ahead of the bisection in every case it measured (2^14 x 64 and
        2^10 x 1024 proofs), but no other group size was timed against it, and the second rule was not measured at all."""
        return default_group_for(protocol, self.k, count)

    def _group_values_packed(self, protocol, rows, sizes, idx, group, wb):
        """(values, status) over the rows idx (a range or a sorted list) in groups of `group` consecutive rows of idx.  A batch beyond
        one call's caps -- 2^16 proofs, ceil(proofs / group) * 2 n <= 2^26 group scalars -- runs as consecutive calls cut at multiples of
        `group`, each under its own slice of the explicit weights wb or a fresh seed."""
        group = int(group)
        if group < 1:
            raise ValueError("group must be at least 1")
        count = len(idx)
        group = min(group, max(count, 1))
        per_w = weight_bytes(protocol)
        groups_per_call = min(max(CALL_MAX // group, 1), max(GROUP_ROWS_MAX // (2 * self.n), 1))
        chunk = groups_per_call * group
        values, status = [], b""
        for lo in range(0, count, chunk):
            hi = min(lo + chunk, count)
            weights = None if wb is None else wb[per_w * lo: per_w * hi]
            seed = None if weights is not None else secrets.token_bytes(32)
            v, st = self.engine.ipa_group_values_packed_dev(self._d[0], self._d[1], self.n, protocol, hi - lo, *packed_rows_cut(protocol, rows, sizes, idx[lo:hi]),
                                                            weights, seed, self._d_scale, group)
            values += v
            status += st
        return values, status

    def group_values_packed2(self, us, Ps, ab, xs, lr, transcripts, starts=None, group=1, weights=None):
        """(values, status) of a packed Protocol-2 batch (the arguments of verify_packed2) per GROUP of `group` consecutive proofs:
        values[t] = the 64-byte value of the weighted combination over the unflagged proofs of [t group, (t + 1) group) -- 64 zero bytes
        when all of them verify --, status[i] = bit 0: proof i fails a byte-level check, bit 1: it has an invalid point (a flagged proof
        takes part in no group).  Never a verdict: the values and the status are the result.  A batch beyond one native call's caps
        (2^16 proofs, ceil(count / group) * 2 n <= 2^26) is cut into consecutive calls at multiples of `group`."""
        rows, sizes, count = self._packed_rows(2, us, Ps, None, ab, xs, lr, None, transcripts, starts)
        return self._group_values_packed(2, rows, sizes, range(count), group, self._weights_bytes(2, weights, count))

    def group_values_packed1(self, u, Ps, cs, ab, xs, lr, head, transcripts, group=1, weights=None):
        """group_values_packed2 for a packed Protocol-1 batch (the arguments of verify_packed1; weights: three per proof)."""
        rows, sizes, count = self._packed_rows(1, u, Ps, cs, ab, xs, lr, head, transcripts, None)
        return self._group_values_packed(1, rows, sizes, range(count), group, self._weights_bytes(1, weights, count))

    def verify_packed2(self, us, Ps, ab, xs, lr, transcripts, starts=None, weights=None):
        """True iff every Protocol-2 proof of the packed batch (ab, xs, lr, transcripts: what prove2_packed returns) is valid for its
        statement (us[i], Ps[i]) -- points or packed bytes, 64 per proof.  starts: Proof2.start_transcript per proof (None: 1, the
        empty prefix).  Random weights come from a fresh 32-byte seed of `secrets` per native call (the soundness note of this
        module applies unchanged); weights: one integer per proof instead, for tests.  A batch above 2^16 proofs runs as consecutive
        calls."""
        rows, sizes, count = self._packed_rows(2, us, Ps, None, ab, xs, lr, None, transcripts, starts)
        return self._verify_packed(2, rows, sizes, count, weights)

    def verify_wire2(self, us, Ps, blobs, off=None, weights=None):
        """True iff every Protocol-2 proof of a batch in the wire format BPIP2 (innerproduct/codec.py) is valid for its statement
        (us[i], Ps[i]) -- points or packed bytes, 64 per proof.  blobs: a list of blobs, or the joined bytes with `off`, count + 1
        offsets (a list or a ctypes array of uint64: what prove2_wire and codec.wire_from_packed return).  ONE native call
        (bpmi_ipa_verify_batch_wire_dev): the bytes are uploaded as they are -- a third of the packed arrays -- and decompressed and
        expanded in device memory; then the work of verify_packed2, unchanged.  A malformed blob or a point that does not decode makes
        the batch invalid.  Weights as verify_packed2; a batch above 2^16 proofs runs as consecutive calls."""
        to_bytes = lambda v: bytes(v) if isinstance(v, (bytes, bytearray, memoryview)) else pack_points(v)
        if off is None:
            blobs, off = split_blobs(blobs)
        count = len(off) - 1
        ub, Pb = to_bytes(us), to_bytes(Ps)
        if count < 0 or len(ub) != 64 * count or len(Pb) != 64 * count:
            raise ValueError("us and Ps: 64 bytes per proof, one per blob")
        wb = self._weights_bytes(2, weights, count)
        for lo in range(0, count, CALL_MAX):               # consecutive calls of at most 2^16 proofs; valid iff every call is
            hi = min(lo + CALL_MAX, count)
            offs = off if hi - lo == count and isinstance(off, ctypes.Array) else (ctypes.c_uint64 * (hi - lo + 1))(*off[lo: hi + 1])
            seed = None if wb is not None else secrets.token_bytes(32)
            out, status = self.engine.ipa_verify_batch_wire_dev(self._d[0], self._d[1], self.n, hi - lo, blobs, offs, ub[64 * lo: 64 * hi], Pb[64 * lo: 64 * hi],
                                                                None if wb is None else wb[32 * lo: 32 * hi], seed, self._d_scale)
            if out != bytes(64) or status != bytes(hi - lo):
                return False
        return True

    def verify_packed1(self, u, Ps, cs, ab, xs, lr, head, transcripts, weights=None):
        """True iff every Protocol-1 proof of the packed batch (ab, xs, lr, head, transcripts: what prove1_packed returns) is valid
        for its statement (u, Ps[i], cs[i]).  weights: three integers (w, r1, r2) per proof instead of the random ones, for tests."""
        rows, sizes, count = self._packed_rows(1, u, Ps, cs, ab, xs, lr, head, transcripts, None)
        return self._verify_packed(1, rows, sizes, count, weights)

    def locate_packed2(self, us, Ps, ab, xs, lr, transcripts, starts=None, group=None):
        """The sorted indices of the invalid proofs of a packed Protocol-2 batch.  group = None or an integer >= 1: the two levels of
        locate.locate_plan over group_values_packed2 -- level 1 is one call with `group` (None: default_group), level 2 one
        call with group = 1 over the unflagged proofs of the groups whose value is not the identity; a valid batch costs one native
        call, a rejected one two.  group = 0: locate_by_bisection over verify calls, every probe one native call over the gathered rows
        of the subset under fresh weights (kept for comparison).  The indices are the same in every case."""
        rows, sizes, count = self._packed_rows(2, us, Ps, None, ab, xs, lr, None, transcripts, starts)
        return self._locate_packed(2, rows, sizes, count, group)

    def locate_packed1(self, u, Ps, cs, ab, xs, lr, head, transcripts, group=None):
        """locate_packed2 for a packed Protocol-1 batch."""
        rows, sizes, count = self._packed_rows(1, u, Ps, cs, ab, xs, lr, head, transcripts, None)
        return self._locate_packed(1, rows, sizes, count, group)


def batch_verify_inner_products(g, h, statements, h_scale=None, engine=None, rng=None):
    """True iff every (u, P, proof2) of `statements` is a valid Protocol-2 proof over g, h."""
    bv = BatchInnerProductVerifier(g, h, h_scale, engine, rng)
    try:
        for u, P, proof2 in statements:
            bv.add(u, P, proof2)
        return bv.verify()
    finally:
        bv.release()
