"""Many inner-product arguments over the same generators, proved in ONE device call (bpmi_ipa_prove_batch;
csrc/ipa_prove_kernels.hpp).  The reference proves one at a time -- a loop of NIProver(g, h, u, P, c, a, b, group, seed).prove()
(reference: src/innerproduct/inner_product_prover.py:11-45) or FastNIProver2(g, h, u, P, a, b, group, transcript).prove() (:48-110)
-- and so do NIProver / FastNIProver2 here: one device state per proof, 2 log n rounds of launches.  Here every protocol step is one
launch over the whole batch, the generators' multiples come from tables built once per prover, and the transcripts are hashed on the
device.  Same proofs, field for field:

    bp = BatchInnerProductProver(g, h, u)
    proofs1 = bp.prove1(Ps, cs, as_, bs, seeds)         # proofs1[i] == NIProver(g, h, u, Ps[i], cs[i], as_[i], bs[i], group, seeds[i]).prove()
    proofs2 = bp.prove2(as_, bs, transcripts)           # proofs2[i] == FastNIProver2(g, h, u, P_i, as_[i], bs[i], group, transcripts[i]).prove()
    Ps = bp.commit(as_, bs)                             # Ps[i] == vector_commitment(g, h, as_[i], bs[i]): prove1's statements, from the same tables
    Ps2 = bp.commit(as_, bs, "inner")                   # ... + <as_[i], bs[i]> * u: the statements of proofs2
    bp.close()

What BatchInnerProductVerifier consumes.  Vectors of 1 .. 1 024 elements (a power of two); longer ones stay with the single-proof
provers, where one proof fills the chip on its own."""
import ctypes

from .. import engine as _engine
from ..ec import Point, pack_points, pack_scalars, secp256k1, unpack_points
from ..utils.utils import ModP
from .inner_product_verifier import Proof1, Proof2

Q = secp256k1.q
MAX_N = 1024                   # PROVER_ELEMS_MAX (csrc/rp_prove_plan_host.hpp): one lane per element, a proof never straddles a block


def _is_bytes(x):
    return isinstance(x, (bytes, bytearray, memoryview))


def _rows(rows, n, what):
    """A list of n-element vectors (ModP / int) or packed bytes (32 little-endian per element, reduced) -> (bytes, count)."""
    if _is_bytes(rows):
        if len(rows) % (32 * n):
            raise ValueError("%s: packed bytes must hold whole vectors of %d scalars" % (what, n))
        return bytes(rows), len(rows) // (32 * n)
    for r in rows:
        if len(r) != n:
            raise ValueError("%s: every vector of this prover has %d elements" % (what, n))
    return b"".join(pack_scalars(r, Q) for r in rows), len(rows)


class BatchInnerProductProver:
    def __init__(self, g, h, u, h_scale=None, engine=None):
        """g, h: lists of points or PackedPoints, n = 2^k <= 1024 each; u: a point.  h_scale: integers c_i -- the arguments then run over
        the generators c_i * h[i] without materialising them (as NIProver(h_scale=...) and BatchInnerProductVerifier(h_scale=...)).
        Builds the fixed-base tables of the 2n + 1 points on the engine's device (engine option prover_table_bits; the default is the
        range prover's: 16-bit windows up to 128 elements -- 302 MB at n = 4, 4.4 GB at n = 64) and keeps them until close()."""
        n = len(g)
        if n < 1 or n & (n - 1) or len(h) != n or (h_scale is not None and len(h_scale) != n):
            raise ValueError("g, h (and h_scale) must have the same power-of-two length")
        if n > MAX_N:
            raise ValueError("the batch prover takes vectors of at most %d elements; longer ones stay with NIProver / FastNIProver2, "
                             "where one proof fills the chip on its own" % MAX_N)
        self.n, self.k = n, n.bit_length() - 1
        self._engine = engine or _engine.default_engine()
        eng = self._engine
        handle = ctypes.c_void_p()
        eng._ck(eng.lib.bpmi_ipa_batch_prover_create(eng.ctx, n, pack_points(g), pack_points(h), u.to_le64(),
                                                     None if h_scale is None else pack_scalars(h_scale, Q), ctypes.byref(handle)))
        self._handle = handle.value

    # ---- packed forms --------------------------------------------------------------------------------------------------------
    def _run(self, protocol, ab, bb, cb, Pb, seeds, count):
        if isinstance(seeds, tuple):
            sb, offs = seeds
            if len(offs) != count + 1:
                raise ValueError("one seed per proof")
            off = offs if isinstance(offs, ctypes.Array) else (ctypes.c_uint64 * (count + 1))(*offs)
        else:
            if len(seeds) != count:
                raise ValueError("one seed per proof")
            off = (ctypes.c_uint64 * (count + 1))()
            pos = 0
            for i, sd in enumerate(seeds):
                off[i] = pos
                pos += len(sd)
            off[count] = pos
            sb = b"".join(seeds)
        if count == 0:
            return b"", b"", b"", b"", []
        eng, k = self._engine, self.k
        longest = max(off[i + 1] - off[i] for i in range(count))
        cap = count * eng.lib.bpmi_ipa_prove_batch_transcript_bytes(self._handle, protocol, longest)
        ab_out = ctypes.create_string_buffer(64 * count)
        xs = ctypes.create_string_buffer(max(32 * k * count, 1))
        lr = ctypes.create_string_buffer(max(128 * k * count, 1))
        head = ctypes.create_string_buffer(128 * count) if protocol == 1 else None
        tr = ctypes.create_string_buffer(cap)
        tr_off = (ctypes.c_uint64 * (count + 1))()
        vp = lambda buf: None if buf is None else ctypes.cast(buf, ctypes.c_void_p)
        eng._ck(eng.lib.bpmi_ipa_prove_batch(self._handle, protocol, count, ab, bb, cb, Pb, sb, off, vp(ab_out), vp(xs), vp(lr), vp(head), vp(tr), cap, tr_off))
        raw = tr.raw
        return (ab_out.raw, xs.raw[: 32 * k * count], lr.raw[: 128 * k * count], head.raw if head is not None else b"",
                [raw[tr_off[i]: tr_off[i + 1]] for i in range(count)])

    def prove1_packed(self, Ps, cs, as_, bs, seeds):
        """Protocol 1 on packed inputs: (ab, xs, LR, head, transcripts) as bpmi_ipa_prove_batch writes them (include/bpmi.h) -- ab 64 B,
        xs 32 k B, LR 128 k B, head 128 B per proof, and the list of the inner transcripts.  Ps: points or packed bytes (64 per proof);
        cs: scalars, packed bytes (32 per proof), or None for c_p = <a_p, b_p>; as_, bs: lists of n-element vectors or packed bytes;
        seeds: a list of bytes, or (joined bytes, offsets)."""
        ab, count = _rows(as_, self.n, "as_")
        bb, count_b = _rows(bs, self.n, "bs")
        Pb = bytes(Ps) if _is_bytes(Ps) else pack_points(Ps)
        cb = None if cs is None else (bytes(cs) if _is_bytes(cs) else pack_scalars(cs, Q))
        if count_b != count or len(Pb) != 64 * count or (cb is not None and len(cb) != 32 * count):
            raise ValueError("Ps, cs, as_ and bs must have the same length")
        return self._run(1, ab, bb, cb, Pb, seeds, count)

    def prove2_packed(self, as_, bs, transcripts=None):
        """Protocol 2 on packed inputs: (ab, xs, LR, transcripts).  transcripts: None (every proof starts from the empty transcript), a
        list of bytes / None, or (joined bytes, offsets)."""
        ab, count = _rows(as_, self.n, "as_")
        bb, count_b = _rows(bs, self.n, "bs")
        if count_b != count:
            raise ValueError("as_ and bs must have the same length")
        if transcripts is None:
            transcripts = [b""] * count
        elif not isinstance(transcripts, tuple):
            transcripts = [t or b"" for t in transcripts]
        out = self._run(2, ab, bb, None, None, transcripts, count)
        return out[0], out[1], out[2], out[4]

    def prove2_wire(self, as_, bs, transcripts=None):
        """Protocol 2 straight to the wire format BPIP2 (innerproduct/codec.py): (blobs, off) -- the proofs of prove2_packed as blobs
        back to back and count + 1 offsets, the arguments of BatchInnerProductVerifier.verify_wire2.  prove2_packed plus the native
        host encoder (bpmi_ipa_wire_encode); start_transcript as prove2 computes it (the items of the prefix, 1 without one)."""
        from .codec import wire_from_packed
        ab, xs, lr, trs = self.prove2_packed(as_, bs, transcripts)
        if isinstance(transcripts, tuple):
            sb, offs = transcripts
            transcripts = [sb[offs[i]: offs[i + 1]] for i in range(len(trs))]
        starts = [len(t.split(b"&")) if t else 1 for t in (transcripts or [None] * len(trs))]
        return wire_from_packed(ab, xs, lr, trs, starts)

    # ---- Proof objects -------------------------------------------------------------------------------------------------------
    def _proof2(self, i, ab, xs, lr, transcript, start):
        k = self.k
        sc = lambda buf, j: ModP(int.from_bytes(buf[32 * j: 32 * j + 32], "little"), Q)
        pts = [Point.from_le64(lr[64 * (2 * k * i + j): 64 * (2 * k * i + j) + 64]) for j in range(2 * k)]
        return Proof2(sc(ab, 2 * i), sc(ab, 2 * i + 1), [sc(xs, k * i + j) for j in range(k)], pts[:k], pts[k:], transcript, start)

    def prove1(self, Ps, cs, as_, bs, seeds):
        """[Proof1]: proof i is NIProver(g, h, u, Ps[i], cs[i], as_[i], bs[i], group, seeds[i]).prove() (reference :29-36)."""
        ab, xs, lr, head, trs = self.prove1_packed(Ps, cs, as_, bs, seeds)
        out = []
        for i, tr in enumerate(trs):
            # the inner transcript is "&" || outer || rounds; the outer one is base64(seed) "&" str(x) "&": items 1 and 2
            items = tr.split(b"&")
            outer = b"&".join(items[1:3]) + b"&"
            p2 = self._proof2(i, ab, xs, lr, tr, len(outer.split(b"&")))
            out.append(Proof1(Point.from_le64(head[128 * i: 128 * i + 64]), Point.from_le64(head[128 * i + 64: 128 * i + 128]), p2, outer))
        return out

    def prove2(self, as_, bs, transcripts=None):
        """[Proof2]: proof i is FastNIProver2(g, h, u, P, as_[i], bs[i], group, transcripts[i]).prove() (reference :56-110; the prover
        never reads P).  start_transcript as the reference computes it (:63-67): the items of the prefix, 1 without one."""
        ab, xs, lr, trs = self.prove2_packed(as_, bs, transcripts)
        if isinstance(transcripts, tuple):
            sb, offs = transcripts
            transcripts = [sb[offs[i]: offs[i + 1]] for i in range(len(trs))]
        starts = [len(t.split(b"&")) if t else 1 for t in (transcripts or [None] * len(trs))]
        return [self._proof2(i, ab, xs, lr, tr, starts[i]) for i, tr in enumerate(trs)]

    # ---- the statements ------------------------------------------------------------------------------------------------------
    def commit_packed(self, as_, bs, u_term=None):
        """The statements of a batch from the prover's tables, in one device call (bpmi_ipa_batch_prover_commit_batch): 64 bytes per
        statement, P_p = sum as_[p][j] g[j] + sum bs[p][j] (h_scale[j] h[j]) + t_p u -- a loop of vector_commitment(g, h, a, b)
        (reference: src/utils/commitments.py:13) plus inner_product(a, b) * u.  as_, bs: lists of n-element vectors or packed bytes,
        either may be None (all zeros).  u_term: None -- no u term, the P that prove1 and Verifier1 take; "inner" -- t_p = <a_p, b_p>
        (over the unscaled b), the P under which prove2's proofs verify; or one scalar per statement, a list or packed bytes."""
        if as_ is None and bs is None:
            raise ValueError("as_ and bs are both None (one of them may be: all zeros)")
        ab, count = (None, None) if as_ is None else _rows(as_, self.n, "as_")
        bb, count_b = (None, None) if bs is None else _rows(bs, self.n, "bs")
        if ab is not None and bb is not None and count_b != count:
            raise ValueError("as_ and bs must have the same length")
        count = count_b if count is None else count
        tb, mode = None, 0
        if isinstance(u_term, str):
            if u_term != "inner":
                raise ValueError('u_term is None, "inner", or one scalar per statement')
            if ab is None or bb is None:
                raise ValueError('u_term = "inner" sums <a, b>: it takes both as_ and bs')
            mode = 1
        elif u_term is not None:
            tb, mode = (bytes(u_term) if _is_bytes(u_term) else pack_scalars(u_term, Q)), 2
            if len(tb) != 32 * count:
                raise ValueError("u_term must hold one scalar per statement")
        if count == 0:
            return b""
        eng = self._engine
        out = ctypes.create_string_buffer(64 * count)
        eng._ck(eng.lib.bpmi_ipa_batch_prover_commit_batch(self._handle, count, ab, bb, mode, tb, ctypes.cast(out, ctypes.c_void_p)))
        return out.raw

    def commit(self, as_, bs, u_term=None):
        """[Point]: commit_packed's statements as points."""
        raw = self.commit_packed(as_, bs, u_term)
        return unpack_points(raw, len(raw) // 64)

    def commit_last_ms(self):
        """Of the last commit: device milliseconds of its kernels, and the whole call (bpmi_ipa_batch_prover_commit_last_ms)."""
        ms = (ctypes.c_double * 2)()
        self._engine._ck(self._engine.lib.bpmi_ipa_batch_prover_commit_last_ms(self._handle, ms))
        return dict(zip(("device", "call"), ms))

    def last_ms(self):
        """Device milliseconds of the last batch by phase (bpmi_ipa_batch_prover_last_ms)."""
        ms = (ctypes.c_double * 4)()
        self._engine._ck(self._engine.lib.bpmi_ipa_batch_prover_last_ms(self._handle, ms))
        return dict(zip(("begin_head", "rounds", "copy_out", "total"), ms))

    def close(self):
        if getattr(self, "_handle", None):
            self._engine.lib.bpmi_ipa_batch_prover_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
