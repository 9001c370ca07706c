"""Range proofs of DIFFERENT sizes from one prover, one table and one device call (csrc/rp_prove_mixed_host.hpp).

MixedBatchRangeVerifier treats a generator list as a capacity: a proof over m amounts uses the first n m generators of one long list.
This is the proving side of the same blocks.  A prover created for (n, M) over gs, hs of n M points serves every CLASS m_c -- a power
of two, 1 <= m_c <= M, n m_c >= 2 -- over gs[:n m_c], hs[:n m_c]: the table of the longest list holds the multiples of every generator
the shorter classes use, and a class reaches them through base lists of its own.  One native call (bpmi_rp_prove_batch_mixed) proves a
list of classes, every protocol step one launch per kernel over all of them.  Each proof is byte for byte what
BatchRangeProver(n, g, h, gs[:n m_c], hs[:n m_c], u, m=m_c) writes -- a loop of AggregNIRangeProver(...).prove()
(/root/reference/src/rangeproofs/rangeproof_aggreg_prover.py:36-146), or of NIRangeProver(...).prove() for m_c = 1
(/root/reference/src/rangeproofs/rangeproof_prover.py:35-91):

    bp = MixedBatchRangeProver(64, g, h, gs, hs, u)                 # gs, hs: 64 x 16 points -> classes m = 1, 2, 4, 8, 16
    out = bp.prove_classes_packed([(1, vs1, gammas1, seeds1), (16, vs16, gammas16, seeds16)])
    cls = [(n_c, bp.commit_packed(vs, gs_), packed, offs) for (n_c, packed, offs), (_, vs, gs_, _) in zip(out, classes)]
    MixedBatchRangeVerifier(g, h, gs, hs, u).partial_packed(cls)    # 64 zero bytes

One window width (the capacity's) serves every class; where that is the right trade against one BatchRangeProver per class is
measured in DESIGN section 6t (tools/bench_rp_prove_mixed.py, profiles/r21_rp_prove_mixed.txt).
"""
import ctypes

from .. import _native
from .. import engine as _engine
from .batch_prover import BatchRangeProver, grown_output, pack_pairs, pack_scalars, seed_offsets


class MixedBatchRangeProver:
    def __init__(self, n, g, h, gs, hs, u, engine=None, wire_format=2):
        """n: bits per value; gs, hs: n M points each, M = len(gs) // n the most values a proof of this prover covers (n and M powers
        of two, 2 <= n M <= 1024).  Builds ONE table over the 3 + 2 n M bases (engine option prover_table_bits; default by n M as for
        BatchRangeProver) and keeps it until close()."""
        if len(gs) != len(hs) or len(gs) % n:
            raise ValueError("gs and hs must have n M points each")
        self.n, self.M, self.wire_format = n, len(gs) // n, wire_format
        self._bp = BatchRangeProver(n, g, h, gs, hs, u, engine=engine, m=self.M, wire_format=wire_format)      # the capacity: its handle, tables and buffers
        self._engine = self._bp._engine
        self._out = None

    def _check_m(self, m):
        if m < 1 or m & (m - 1) or m > self.M or self.n * m < 2:
            raise ValueError("a class has a power of two of values per proof, at most %d, with bits x values >= 2" % self.M)

    def commit_packed(self, vs, gammas):
        """The commitments V = v g + gamma h, 64 bytes per value, in the order given (the tables of g and h do not depend on the class):
        vs, gammas as packed bytes, flat lists, or lists of rows."""
        vb, gb = pack_scalars(vs), pack_scalars(gammas)
        if len(vb) != len(gb) or len(vb) % 32:
            raise ValueError("values and blinding factors must have the same length")
        out = ctypes.create_string_buffer(max(2 * len(vb), 1))
        eng = self._engine
        eng._ck(eng.lib.bpmi_rp_prover_commit_batch(self._bp._handle, len(vb) // 32, vb, gb, ctypes.cast(out, ctypes.c_void_p)))
        return out.raw[: 2 * len(vb)]

    def commit(self, vs, gammas):
        """The same as Points, shaped like vs (a list of rows gives a list of rows)."""
        from ..ec import Point
        raw = self.commit_packed(vs, gammas)
        pts = [Point.from_le64(raw[o: o + 64]) for o in range(0, len(raw), 64)]
        if not isinstance(vs, (bytes, bytearray, memoryview)) and len(vs) and isinstance(vs[0], (list, tuple)):
            out, at = [], 0
            for row in vs:
                out.append(pts[at: at + len(row)])
                at += len(row)
            return out
        return pts

    def prove_classes_packed(self, classes, copy=True):
        """classes = [(m_c, vs, gammas, seeds)] in the forms BatchRangeProver.prove_wire_packed takes (lists of ModP / int -- rows of m_c
        per proof -- or packed bytes; seeds a list of bytes or (joined bytes, offsets)) -> [(n_c, packed_c, offsets_c)], n_c = n m_c
        the class's generators, proof i of class c = packed_c[offsets_c[i]: offsets_c[i + 1]].  With commit_packed a result is one class
        tuple of MixedBatchRangeVerifier.partial_packed / group_values_packed.  copy=False: packed_c are memoryviews of the prover's
        page-locked output buffer, valid until the next call or close()."""
        eng = self._engine
        arr = (_native.RpProveClass * max(len(classes), 1))()
        keep, counts, total, cap = [], [], 0, 16
        eng.set_option("prover_wire_format", self.wire_format)
        for c, (m, vs, gammas, seeds) in enumerate(classes):
            self._check_m(m)
            vb, gb, cnt = pack_pairs(vs, gammas, m, "class")
            sb, off = seed_offsets(seeds, cnt)
            keep += [vb, gb, sb, off]
            arr[c].m, arr[c].n_proofs = m, cnt
            arr[c].values, arr[c].gammas = ctypes.cast(ctypes.c_char_p(vb), ctypes.c_void_p), ctypes.cast(ctypes.c_char_p(gb), ctypes.c_void_p)
            arr[c].seeds, arr[c].seed_off = ctypes.cast(ctypes.c_char_p(sb), ctypes.c_void_p), ctypes.addressof(off)
            cap += cnt * eng.lib.bpmi_rp_prove_batch_proof_bytes_class(self._bp._handle, m, 0) + (off[cnt] - off[0])
            counts.append(cnt)
            total += cnt
        self._out = grown_output(eng, self._out, cap)
        out_off = (ctypes.c_uint64 * (total + 1))()
        eng._ck(eng.lib.bpmi_rp_prove_batch_mixed(self._bp._handle, len(classes), ctypes.cast(arr, ctypes.c_void_p), ctypes.c_void_p(self._out.ptr), cap,
                                                  ctypes.cast(out_off, ctypes.c_void_p)))
        del keep
        res, first = [], 0
        for (m, _, _, _), cnt in zip(classes, counts):
            lo, hi = out_off[first], out_off[first + cnt]
            view = self._out.view[lo: hi]
            res.append((self.n * m, view if not copy else bytes(view), [out_off[first + i] - lo for i in range(cnt + 1)]))
            first += cnt
        return res

    def prove_wire(self, items):
        """items = [(vs_i, gammas_i, seed_i)] in any order, vs_i / gammas_i lists of m_i values (a single ModP / int: m_i = 1) -> the wire
        proofs in the items' order.  The classes are formed by a stable sort on m_i, as MixedBatchRangeVerifier.classes forms them."""
        items = [(list(v) if isinstance(v, (list, tuple)) else [v], list(gm) if isinstance(gm, (list, tuple)) else [gm], sd) for v, gm, sd in items]
        for v, gm, _ in items:
            if len(v) != len(gm):
                raise ValueError("values and blinding factors must have the same length")
            self._check_m(len(v))
        order = sorted(range(len(items)), key=lambda i: len(items[i][0]))          # (stable)
        classes, members = [], []
        for i in order:
            m = len(items[i][0])
            if not classes or classes[-1][0] != m:
                classes.append((m, [], [], []))
                members.append([])
            classes[-1][1].append(items[i][0])
            classes[-1][2].append(items[i][1])
            classes[-1][3].append(items[i][2])
            members[-1].append(i)
        out = [None] * len(items)
        for (_, packed, offs), idx in zip(self.prove_classes_packed(classes), members):
            for j, i in enumerate(idx):
                out[i] = packed[offs[j]: offs[j + 1]]
        return out

    def last_ms(self):
        """Device milliseconds of the last call by phase (bpmi_rp_prover_last_ms: the seven phases of BatchRangeProver.last_ms)."""
        return self._bp.last_ms()

    def close(self):
        if getattr(self, "_bp", None) is not None:
            self._bp.close()
        if getattr(self, "_out", None) is not None:
            self._out.free()
            self._out = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
