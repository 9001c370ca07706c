"""Inner-product arguments of DIFFERENT lengths from one prover, one table and one device call (csrc/ipa_prove_mixed_host.hpp).

MixedBatchInnerProductVerifier treats a generator list as a capacity: a statement over n_c elements uses g[:n_c], h[:n_c] of one long
list.  This is the proving side of the same blocks.  A prover created over N generators serves every CLASS n_c = 2^k_c <= N over the
prefixes g[:n_c], h[:n_c] (and h_scale[:n_c]) with the one u: the rounds never fold a generator, so the table of the longest list holds
every multiple the shorter classes use, and a class reaches them through base lists of its own.  One native call
(bpmi_ipa_prove_batch_mixed) proves a list of classes, every protocol step one launch per kernel over all of them.  Each proof is byte
for byte what BatchInnerProductProver(g[:n_c], h[:n_c], u) writes -- a loop of NIProver(...).prove()
(reference: src/innerproduct/inner_product_prover.py:11-45) or of FastNIProver2(...).prove() (:48-110) over that prefix:

    bp = MixedBatchInnerProductProver(g, h, u)                       # g, h: 1 024 points -> classes n = 1, 2, 4, ... 1 024
    out = bp.prove2_classes_packed([(64, as64, bs64, None), (1024, as1k, bs1k, None)])
    Ps = bp.commit_classes_packed([(64, as64, bs64), (1024, as1k, bs1k)], "inner")
    cls = [(u, P) + o for P, o in zip(Ps, out)]                      # the class tuples of MixedBatchInnerProductVerifier.verify_packed2
    bp.close()

Which call for which block is measured in DESIGN.md section 6v (tools/bench_ipa_prove_mixed.py, profiles/r22_ipa_prove_mixed.txt);
one window width (the capacity's) serves every class.
"""
import ctypes

from .. import _native
from ..ec import Point, pack_points, pack_scalars
from .batch_prover import BatchInnerProductProver, Q, _is_bytes, _rows
from ..utils.utils import ModP
from .inner_product_verifier import Proof1, Proof2


def _addr(b):
    return None if b is None else ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p)


def _seed_offsets(seeds, count):
    """a list of bytes / None, or (joined bytes, offsets) -> (joined bytes, a c_uint64 array of count + 1 offsets)"""
    if isinstance(seeds, tuple):
        sb, offs = seeds
        if len(offs) != count + 1:
            raise ValueError("one seed per proof")
        return bytes(sb), (offs if isinstance(offs, ctypes.Array) else (ctypes.c_uint64 * (count + 1))(*offs))
    if len(seeds) != count:
        raise ValueError("one seed per proof")
    off = (ctypes.c_uint64 * (count + 1))()
    pos = 0
    for i, sd in enumerate(seeds):
        off[i] = pos
        pos += len(sd or b"")
    off[count] = pos
    return b"".join(sd or b"" for sd in seeds), off


class MixedBatchInnerProductProver:
    """Which call for which block (measured: profiles/r22_ipa_prove_mixed.txt; Protocol 2, lengths 64 .. 1 024,
    against one BatchInnerProductProver per length).  Up to 64 proofs per length: this class -- 21-22 ms against 35 ms, the loop pays five
    latency chains and this call one -- with ONE 5.9 GB table against five of 29.3 GB.  At 2 048 / 1 024 / 512 / 256 / 256 proofs this
    class LOSES: 51 ms against 43 ms for the loop at its default window widths (19 % slower) and 45 ms for the loop at this table's 12
    bits (13 %); there it is the call for where the table memory is not to be spent.  The crossover between 64 and 2 048 proofs per
    length was not measured."""

    def __init__(self, g, h, u, h_scale=None, engine=None):
        """g, h: N = 2^K <= 1024 points each, the capacity; u: a point; h_scale: N integers or None, as BatchInnerProductProver takes
        them.  Builds ONE table over the 2 N + 1 bases (engine option prover_table_bits; default by N) and keeps it until close()."""
        self._bp = BatchInnerProductProver(g, h, u, h_scale=h_scale, engine=engine)      # the capacity: its handle, table and buffers
        self.n, self.k = self._bp.n, self._bp.k
        self._engine = self._bp._engine

    def _check_n(self, n):
        if n < 1 or n & (n - 1) or n > self.n:
            raise ValueError("a class has a power-of-two vector length of at most %d" % self.n)

    # ---- packed forms --------------------------------------------------------------------------------------------------------
    def _run(self, protocol, classes):
        """classes: [(n, count, a, b, c, P, seeds)] with packed inputs -> [(ab, xs, lr, head, transcripts)]"""
        eng, handle = self._engine, self._bp._handle
        arr = (_native.IpaProveClass * max(len(classes), 1))()
        keep, outs = [], []
        for c, (n, count, ab, bb, cb, Pb, seeds) in enumerate(classes):
            k = n.bit_length() - 1
            sb, off = _seed_offsets(seeds, count)
            longest = max(off[i + 1] - off[i] for i in range(count))
            cap = count * eng.lib.bpmi_ipa_prove_batch_transcript_bytes_class(handle, n, protocol, longest)
            o = dict(ab=ctypes.create_string_buffer(64 * count), xs=ctypes.create_string_buffer(max(32 * k * count, 1)),
                     LR=ctypes.create_string_buffer(max(128 * k * count, 1)), head=ctypes.create_string_buffer(128 * count) if protocol == 1 else None,
                     transcripts=ctypes.create_string_buffer(max(cap, 1)), tr_off=(ctypes.c_uint64 * (count + 1))())
            keep += [ab, bb, cb, Pb, sb, off]
            q = arr[c]
            q.n, q.n_proofs, q.cap = n, count, cap
            q.a, q.b, q.c, q.P, q.seeds = _addr(ab), _addr(bb), _addr(cb), _addr(Pb), _addr(sb)
            q.seed_off = ctypes.addressof(off)
            for name in ("ab", "xs", "LR", "head", "transcripts"):
                setattr(q, name, None if o[name] is None else ctypes.addressof(o[name]))
            q.tr_off = ctypes.addressof(o["tr_off"])
            outs.append((k, count, o))
        eng._ck(eng.lib.bpmi_ipa_prove_batch_mixed(handle, protocol, len(classes), ctypes.cast(arr, ctypes.c_void_p)))
        del keep
        res = []
        for k, count, o in outs:
            raw, tr_off = o["transcripts"].raw, o["tr_off"]
            res.append((o["ab"].raw, o["xs"].raw[: 32 * k * count], o["LR"].raw[: 128 * k * count], o["head"].raw if o["head"] is not None else b"",
                        [raw[tr_off[i]: tr_off[i + 1]] for i in range(count)]))
        return res

    def _vectors(self, n, as_, bs):
        self._check_n(n)
        ab, count = _rows(as_, n, "as_")
        bb, count_b = _rows(bs, n, "bs")
        if count_b != count or count == 0:
            raise ValueError("as_ and bs of a class must have the same length, at least 1")
        return ab, bb, count

    def prove2_classes_packed(self, classes):
        """Protocol 2: classes = [(n_c, as_, bs, transcripts)] in the forms BatchInnerProductProver.prove2_packed takes -> per class
        (ab, xs, lr, transcripts), what prove2_packed of a prover over the prefix returns."""
        packed = []
        for n, as_, bs, transcripts in classes:
            ab, bb, count = self._vectors(n, as_, bs)
            packed.append((n, count, ab, bb, None, None, [b""] * count if transcripts is None else transcripts))
        return [(o[0], o[1], o[2], o[4]) for o in self._run(2, packed)]

    def prove1_classes_packed(self, classes):
        """Protocol 1: classes = [(n_c, Ps, cs, as_, bs, seeds)] in the forms of prove1_packed (cs None per class: c_p = <a_p, b_p>) ->
        per class (ab, xs, lr, head, transcripts)."""
        packed = []
        for n, Ps, cs, as_, bs, seeds in classes:
            ab, bb, count = self._vectors(n, as_, bs)
            Pb = bytes(Ps) if _is_bytes(Ps) else pack_points(Ps)
            cb = None if cs is None else (bytes(cs) if _is_bytes(cs) else pack_scalars(cs, Q))
            if len(Pb) != 64 * count or (cb is not None and len(cb) != 32 * count):
                raise ValueError("Ps, cs, as_ and bs must have the same length")
            packed.append((n, count, ab, bb, cb, Pb, seeds))
        return self._run(1, packed)

    def commit_classes_packed(self, classes, u_term=None):
        """The statements of the classes from the prover's table in one call (bpmi_ipa_batch_prover_commit_batch_mixed): classes =
        [(n_c, as_, bs[, ts])] -> [bytes], 64 per statement, what BatchInnerProductProver.commit_packed of a prover over the prefix
        returns.  u_term for the whole call: None, "inner", or "given" with one scalar per statement in ts (a list or packed bytes).
        as_ or bs of a class may be None (all zeros), not both, and not under "inner"."""
        if u_term not in (None, "inner", "given"):
            raise ValueError('u_term is None, "inner" or "given"')
        mode = {None: 0, "inner": 1, "given": 2}[u_term]
        eng = self._engine
        arr = (_native.IpaCommitClass * max(len(classes), 1))()
        keep, outs = [], []
        for c, cl in enumerate(classes):
            n, as_, bs = cl[:3]
            self._check_n(n)
            if as_ is None and bs is None:
                raise ValueError("as_ and bs are both None (one of them may be: all zeros)")
            ab, count = (None, None) if as_ is None else _rows(as_, n, "as_")
            bb, count_b = (None, None) if bs is None else _rows(bs, n, "bs")
            if ab is not None and bb is not None and count_b != count:
                raise ValueError("as_ and bs must have the same length")
            count = count_b if count is None else count
            if mode == 1 and (ab is None or bb is None):
                raise ValueError('u_term = "inner" sums <a, b>: it takes both as_ and bs')
            tb = None
            if mode == 2:
                if len(cl) < 4:
                    raise ValueError('u_term = "given" takes (n, as_, bs, ts)')
                tb = bytes(cl[3]) if _is_bytes(cl[3]) else pack_scalars(cl[3], Q)
                if len(tb) != 32 * count:
                    raise ValueError("ts must hold one scalar per statement")
            out = ctypes.create_string_buffer(max(64 * count, 1))
            keep += [ab, bb, tb]
            q = arr[c]
            q.n, q.count, q.a, q.b, q.t, q.out = n, count, _addr(ab), _addr(bb), _addr(tb), ctypes.addressof(out)
            outs.append((count, out))
        eng._ck(eng.lib.bpmi_ipa_batch_prover_commit_batch_mixed(self._bp._handle, mode, len(classes), ctypes.cast(arr, ctypes.c_void_p)))
        del keep
        return [out.raw[: 64 * count] for count, out in outs]

    # ---- Proof objects over items of any lengths ---------------------------------------------------------------------------------
    @staticmethod
    def _classes_of(lengths):
        """a stable sort on the length: [(n, [item indices])], as MixedBatchInnerProductVerifier forms its classes"""
        groups = []
        for i in sorted(range(len(lengths)), key=lambda i: lengths[i]):
            if not groups or groups[-1][0] != lengths[i]:
                groups.append((lengths[i], []))
            groups[-1][1].append(i)
        return groups

    @staticmethod
    def _proof2(k, i, ab, xs, lr, transcript, start):
        """proof i of a class of k rounds from its packed arrays (BatchInnerProductProver._proof2 with the class's k)"""
        sc = lambda buf, j: ModP(int.from_bytes(buf[32 * j: 32 * j + 32], "little"), Q)
        pts = [Point.from_le64(lr[64 * (2 * k * i + j): 64 * (2 * k * i + j) + 64]) for j in range(2 * k)]
        return Proof2(sc(ab, 2 * i), sc(ab, 2 * i + 1), [sc(xs, k * i + j) for j in range(k)], pts[:k], pts[k:], transcript, start)

    def prove2(self, items):
        """items = [(a_i, b_i, transcript_i)] in any order (transcript_i bytes or None; len(a_i) is the item's length) -> [Proof2] in
        the items' order: proof i is FastNIProver2(g[:n_i], h[:n_i], u, P, a_i, b_i, group, transcript_i).prove().  start_transcript as
        BatchInnerProductProver.prove2 computes it."""
        for a, b, _ in items:
            if len(a) != len(b):
                raise ValueError("a and b of an item must have the same length")
            self._check_n(len(a))
        groups = self._classes_of([len(a) for a, _, _ in items])
        got = self.prove2_classes_packed([(n, [items[i][0] for i in idx], [items[i][1] for i in idx], [items[i][2] for i in idx]) for n, idx in groups])
        out = [None] * len(items)
        for (n, idx), (ab, xs, lr, trs) in zip(groups, got):
            for j, i in enumerate(idx):
                t = items[i][2]
                out[i] = self._proof2(n.bit_length() - 1, j, ab, xs, lr, trs[j], len(t.split(b"&")) if t else 1)
        return out

    def prove1(self, items):
        """items = [(P_i, c_i, a_i, b_i, seed_i)] in any order -> [Proof1] in the items' order: proof i is NIProver(g[:n_i], h[:n_i], u,
        P_i, c_i, a_i, b_i, group, seed_i).prove()."""
        for _, _, a, b, _ in items:
            if len(a) != len(b):
                raise ValueError("a and b of an item must have the same length")
            self._check_n(len(a))
        groups = self._classes_of([len(it[2]) for it in items])
        got = self.prove1_classes_packed([(n, [items[i][0] for i in idx], [items[i][1] for i in idx], [items[i][2] for i in idx], [items[i][3] for i in idx],
                                           [items[i][4] for i in idx]) for n, idx in groups])
        out = [None] * len(items)
        for (n, idx), (ab, xs, lr, head, trs) in zip(groups, got):
            for j, i in enumerate(idx):
                parts = trs[j].split(b"&")
                outer = b"&".join(parts[1:3]) + b"&"             # base64(seed) "&" str(x) "&": BatchInnerProductProver.prove1
                p2 = self._proof2(n.bit_length() - 1, j, ab, xs, lr, trs[j], len(outer.split(b"&")))
                out[i] = Proof1(Point.from_le64(head[128 * j: 128 * j + 64]), Point.from_le64(head[128 * j + 64: 128 * j + 128]), p2, outer)
        return out

    def last_ms(self):
        """Device milliseconds of the last proving call by phase (bpmi_ipa_batch_prover_last_ms: the four phases of BatchInnerProductProver.last_ms)."""
        return self._bp.last_ms()

    def commit_last_ms(self):
        """Of the last statements call: device milliseconds of its kernels, and the whole call (bpmi_ipa_batch_prover_commit_last_ms)."""
        return self._bp.commit_last_ms()

    def close(self):
        if getattr(self, "_bp", None) is not None:
            self._bp.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
