"""Batch verification of range proofs of DIFFERENT sizes in one MSM.

A block of transactions carries proofs over 1, 2, 4 ... amounts: AggregNIRangeProver proofs of m values of 64 bits over the FIRST 64 m
generators of one long list.  Every verification equation (rangeproofs.batch) is linear in g, h, u, gs_i, hs_i, and a proof over n_c
generators only touches the indices i < n_c -- so the shared coefficients of proofs of every size add up, prefix by prefix, into the
coefficients of the longest list, and the whole block is ONE combination that must be the identity.

A CLASS is the run of a call's proofs with the same (k = log2 n_gens, m = values per proof, wire format).  The device path is one
native call (bpmi_rp_batch_verify_mixed_dev, csrc/rp_mixed_dev_host.hpp): every class prepared in its own regions, the two latency-bound
chain kernels launched once for all classes, the classes' coefficients merged on the device, one MSM.  Proofs are numbered class-major
over the call; that global index selects a proof's weights.

Measured (tools/bench_rp_verify_mixed.py, profiles/r13_rp_verify_mixed.txt): 2^12 distinct proofs of 1 / 2 / 4 / 8 / 16
values of 64 bits in 1.55 ms through partial_packed against 3.6-3.7 ms for the loop of BatchRangeVerifier.partial_wire per class plus
ec_sum on the same build; the preparation stages take 1.2 ms of device time against 2.3 summed over the loop.  partial_wire(items)
adds Python work per item (grouping, packing) on top of that; a caller that holds its classes packed uses partial_packed.
"""
import ctypes
import os
from itertools import accumulate

from .. import _native
from .. import engine as _engine
from .batch import _ZERO64, BatchRangeVerifier

_FORMATS = b"123"


class MixedBatchRangeVerifier:
    def __init__(self, g, h, gs, hs, u, msm=None, rng=None, engine=None, decompress=None):
        """g, h, u and the LONGEST generator lists gs, hs: a proof over n generators uses gs[:n], hs[:n].
        msm / rng / engine as for BatchRangeVerifier.  With msm= (and decompress=, the stand-in of the engine's point decompression) the
        host path runs: per class add_wire_native(prepare="host") on a verifier over the prefix, then BatchRangeVerifier.merge_prefix."""
        assert len(gs) == len(hs)
        self.g, self.h, self.gs, self.hs, self.u = g, h, list(gs), list(hs), u
        self.N = len(self.gs)
        self._msm, self._rng, self._engine, self._decompress = msm, rng, engine, decompress
        self._shared_pts = g.to_le64() + h.to_le64() + u.to_le64() + b"".join(p.to_le64() for p in self.gs) + b"".join(p.to_le64() for p in self.hs)
        self._d_gens = None
        self._bufs = None
        self._prefix = {}

    def _eng(self):
        return self._engine or _engine.default_engine()

    def release(self):
        """Free every device buffer this verifier and its per-class verifiers hold."""
        if self._d_gens is not None:
            self._d_gens.free()
            self._d_gens = None
        if self._bufs is not None:
            self._bufs[1].free()
            self._bufs[2].free()
            self._bufs = None
        for bv in self._prefix.values():
            bv.release()
        self._prefix = {}

    def prefix_verifier(self, n):
        """The BatchRangeVerifier over gs[:n], hs[:n] (kept: its generators are uploaded once)."""
        bv = self._prefix.get(n)
        if bv is None:
            bv = BatchRangeVerifier(self.g, self.h, self.gs[:n], self.hs[:n], self.u, msm=self._msm, rng=self._rng, engine=self._engine)
            self._prefix[n] = bv
        return bv

    def classes(self, items):
        """items: (V or [V_0 .. V_{m-1}], wire proof) in any order -> [(n_gens, m, format, [indices into items])], the classes in the
        order of a stable sort on (k, m, format).  The size of a proof is read from its k byte, m from its commitments; a proof that is
        too short to have them, a k above this verifier's list or an m that does not divide 2^k raises Exception("Proof invalid")."""
        keys = []
        for V, blob in items:
            m = len(V) if isinstance(V, (list, tuple)) else 1
            if len(blob) < 6 or bytes(blob[:4]) != b"BPRP" or blob[4] not in _FORMATS:
                raise Exception("Proof invalid")
            k = blob[5]
            if k < 1 or k > 16 or (1 << k) > self.N or m < 1 or (1 << k) % m:
                raise Exception("Proof invalid")
            keys.append((k, m, blob[4]))
        order = sorted(range(len(items)), key=keys.__getitem__)          # (stable)
        out = []
        for i in order:
            k, m, fmt = keys[i]
            if not out or out[-1][:3] != (1 << k, m, fmt):
                out.append((1 << k, m, fmt, []))
            out[-1][3].append(i)
        return out

    @staticmethod
    def _commitments(V):
        return list(V) if isinstance(V, (list, tuple)) else [V]

    def _weights(self, count):
        """Explicit weights (4 per proof, global order) when an rng was given, else a fresh seed: (weights, seed)."""
        if self._rng is None:
            return None, os.urandom(32)
        from .batch import Q
        return b"".join(((self._rng() % Q) or 1).to_bytes(32, "little") for _ in range(4 * count)), None

    def partial_wire(self, items):
        """The 64-byte value of the ONE combination over every proof of `items` (64 zero bytes = all valid); raises
        Exception("Proof invalid") when a proof fails a byte-level check or has an invalid point."""
        items = list(items)
        if not items:
            return _ZERO64
        classes = self.classes(items)
        if self._msm is not None:
            return self._partial_host(items, classes)
        packed = []
        for n, m, _, idx in classes:
            packed.append((n, b"".join(P.to_le64() for i in idx for P in self._commitments(items[i][0])), [bytes(items[i][1]) for i in idx], None))
        return self.partial_packed(packed)

    def partial_packed(self, classes):
        """partial_wire for a caller that holds its classes already: [(n_gens, commitments packed (count_c x m x 64 bytes), blobs, offsets)]
        in the call's class order, blobs / offsets as for BatchRangeVerifier.partial_wire (a list of wire proofs with offsets = None, or one
        bytes object with count_c + 1 offsets); m is read from the commitments' length.  No Python work per proof.  Device path only."""
        if self._msm is not None:
            raise ValueError("partial_packed needs the default engine (no custom msm)")
        eng = self._eng()
        if self._d_gens is None or self._d_gens.engine is not eng:
            self._d_gens = eng.upload(self._shared_pts)
        keep, arr = [], (_native.RpClass * max(len(classes), 1))()
        npairs = total = 0
        for c, (n, vb, blobs, offsets) in enumerate(classes):
            if offsets is None:
                cnt = len(blobs)
                offs = (ctypes.c_uint64 * (cnt + 1))(0, *accumulate(map(len, blobs)))
                joined = b"".join(blobs)
            else:
                cnt = len(offsets) - 1
                offs = offsets if isinstance(offsets, ctypes.Array) else (ctypes.c_uint64 * (cnt + 1))(*offsets)
                joined = bytes(blobs)
                if cnt < 1 or not (0 <= offs[0] and offs[cnt] <= len(joined)):
                    raise ValueError("offsets must be non-decreasing positions inside the %d-byte proof buffer" % len(joined))
            vb = bytes(vb)
            m = len(vb) // (64 * cnt) if cnt else 0
            if m < 1 or len(vb) != 64 * cnt * m or n % m:
                raise Exception("Proof invalid")
            keep += [offs, joined, vb]
            arr[c].n_gens, arr[c].values_per_proof, arr[c].n_proofs = n, m, cnt
            arr[c].blobs, arr[c].blobs_len = ctypes.cast(ctypes.c_char_p(joined), ctypes.c_void_p), len(joined)
            arr[c].blob_off, arr[c].v_points = ctypes.addressof(offs), ctypes.cast(ctypes.c_char_p(vb), ctypes.c_void_p)
            npairs += cnt * (m + 6 + 2 * max(n.bit_length() - 1, 0))
            total += cnt
        bufs = self._bufs
        if bufs is None or bufs[0] < npairs or bufs[1].engine is not eng:
            if bufs is not None:
                bufs[1].free()
                bufs[2].free()
            bufs = self._bufs = (npairs, eng.alloc(64 * max(npairs, 1)), eng.alloc(32 * max(npairs, 1)))
        weights, seed = self._weights(total)
        out = ctypes.create_string_buffer(64)
        bad = ctypes.c_int64(-1)
        eng._ck(eng.lib.bpmi_rp_batch_verify_mixed_dev(eng.ctx, len(classes), ctypes.cast(arr, ctypes.c_void_p), self.N, weights, seed, self._d_gens.ptr,
                                                       bufs[1].ptr, bufs[2].ptr, out, ctypes.cast(ctypes.pointer(bad), ctypes.c_void_p)))
        del keep
        if bad.value >= 0:
            raise Exception("Proof invalid")
        return out.raw

    def _partial_host(self, items, classes):
        """The host path: the classes in order (so that an rng's weights follow the global index), each prepared by
        bpmi_rp_batch_prepare on a verifier over its prefix and merged with merge_prefix; one MSM through `msm`."""
        full = BatchRangeVerifier(self.g, self.h, self.gs, self.hs, self.u, msm=self._msm, rng=self._rng, engine=self._engine)
        for n, m, _, idx in classes:
            bv = self.prefix_verifier(n)
            bv.reset()
            Vs = [self._commitments(items[i][0]) for i in idx]
            bv.add_wire_native(Vs if m > 1 else [v[0] for v in Vs], [bytes(items[i][1]) for i in idx], decompress=self._decompress, prepare="host")
            full.merge_prefix(bv.state())
            bv.reset()
        return full.partial()

    def verify_wire(self, items, sharded=None):
        """True if every proof of `items` is valid; raises Exception("Proof invalid") otherwise (`sharded`: a distributed.ShardedMSM that
        folds the ranks' values first)."""
        part = self.partial_wire(items)
        if sharded is not None:
            part = sharded.combine(part)
        if part != _ZERO64:
            raise Exception("Proof invalid")
        return True

    def locate_wire(self, items):
        """The sorted indices, in the CALLER's order, of every invalid proof of `items`; [] for a valid batch.  Class by class through
        BatchRangeVerifier.locate_wire of the verifier over the class's prefix (a device group mode for mixed batches does not exist).
        A proof whose size cannot be read, or does not fit this verifier, is invalid."""
        items = list(items)
        bad, sound = [], []
        for i, it in enumerate(items):
            try:
                self.classes([it])
                sound.append(i)
            except Exception:
                bad.append(i)
        for n, m, _, idx in self.classes([items[i] for i in sound]):
            idx = [sound[j] for j in idx]
            Vs = [self._commitments(items[i][0]) for i in idx]
            found = self.prefix_verifier(n).locate_wire(Vs if m > 1 else [v[0] for v in Vs], [bytes(items[i][1]) for i in idx])
            bad += [idx[j] for j in found]
        return sorted(bad)
