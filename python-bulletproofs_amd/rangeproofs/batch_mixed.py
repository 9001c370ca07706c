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

Which proofs of a rejected block are invalid: locate_wire(items) goes class by class; locate_wire(items, group=None) is two native calls
over all classes (bpmi_rp_batch_group_values_mixed_dev through group_values_packed; DESIGN section 6s, profiles/r20_rp_locate_mixed.txt).
"""
import ctypes
import os
from itertools import accumulate

from .. import _native
from .. import engine as _engine
from ..locate import locate_plan_groups
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
        return self.partial_packed(self._packed_items(items, classes))

    def partial_packed(self, classes):
        """partial_wire for a caller that holds its classes already: [(n_gens, commitments packed (count_c x m x 64 bytes), blobs, offsets)]
        in the call's class order, blobs / offsets as for BatchRangeVerifier.partial_wire (a list of wire proofs with offsets = None, or one
        bytes object with count_c + 1 offsets); m is read from the commitments' length.  No Python work per proof.  Device path only."""
        eng, arr, keep, counts, bufs = self._native_classes("partial_packed", classes)
        weights, seed = self._weights(sum(counts))
        out = ctypes.create_string_buffer(64)
        bad = ctypes.c_int64(-1)
        eng._ck(eng.lib.bpmi_rp_batch_verify_mixed_dev(eng.ctx, len(classes), ctypes.cast(arr, ctypes.c_void_p), self.N, weights, seed, self._d_gens.ptr,
                                                       bufs[1].ptr, bufs[2].ptr, out, ctypes.cast(ctypes.pointer(bad), ctypes.c_void_p)))
        del keep
        if bad.value >= 0:
            raise Exception("Proof invalid")
        return out.raw

    def _native_classes(self, what, classes):
        """The packed classes of partial_packed / group_values_packed as the native calls take them: (engine, the array of RpClass, the
        objects its addresses point into, the classes' proof counts, the scratch buffers); the generators are uploaded once."""
        if self._msm is not None:
            raise ValueError("%s needs the default engine (no custom msm)" % what)
        eng = self._eng()
        if self._d_gens is None or self._d_gens.engine is not eng:
            self._d_gens = eng.upload(self._shared_pts)
        keep, arr = [], (_native.RpClass * max(len(classes), 1))()
        npairs, counts = 0, []
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
            counts.append(cnt)
        bufs = self._bufs
        if bufs is None or bufs[0] < npairs or bufs[1].engine is not eng:
            if bufs is not None:
                bufs[1].free()
                bufs[2].free()
            bufs = self._bufs = (npairs, eng.alloc(64 * max(npairs, 1)), eng.alloc(32 * max(npairs, 1)))
        return eng, arr, keep, counts, bufs

    # ---- per GROUP of consecutive proofs of one class: one native call names the groups that hold an invalid proof ----------------------
    # bpmi_rp_batch_group_values_mixed_dev (csrc/rp_group_mixed_dev_host.hpp): the mixed preparation once, the cells summed per group, the
    # groups' MSMs over [g h u gs[:n_c] hs[:n_c] | the group's commitments | the group's proof points] in at most one launch per block
    # shape.  locate_wire(items, group=None | >= 1 | list) is two such calls (locate.locate_plan_groups).
    @staticmethod
    def _class_groups(group, n_classes):
        """`group` as one integer >= 1 per class: an integer for every class, or a list with one per class."""
        groups = [int(g) for g in group] if isinstance(group, (list, tuple)) else [int(group)] * n_classes
        if len(groups) != n_classes or any(g < 1 for g in groups):
            raise ValueError("group: an integer >= 1, or a list with one integer >= 1 per class")
        return groups

    def default_groups(self, shapes):
        """The group sizes locate_wire starts with under group=None: per class (n_gens, m) the default_group(m) of the verifier over its
        prefix -- the largest power of two whose group fits one launch of the group kernel (a capacity rule, not a measured optimum)."""
        return [self.prefix_verifier(n).default_group(m) for n, m in shapes]

    def group_values_packed(self, classes, groups):
        """(values, value_off, status) of the packed classes (the argument of partial_packed, no class empty) per GROUP of consecutive
        proofs of one class.  groups: one integer >= 1 per class; class c is cut into groups of min(groups[c], count_c) proofs, the last
        one possibly short, and owns values[value_off[c]: value_off[c + 1]] -- a group never straddles a class.  values[t] = the 64-byte
        value of the combination over the unflagged proofs of group t over the prefix of its class (64 zero bytes: all of them verify),
        status[i] (global, class-major index) = bit 0: proof i fails a byte-level check, bit 1: it has an invalid point encoding (a
        flagged proof takes part in no group).  Never raises "Proof invalid": the values and the status are the result.  No Python work
        per proof.  Device path only."""
        classes = list(classes)
        groups = [int(g) for g in groups]
        if len(groups) != len(classes):
            raise ValueError("one group size per class")
        if not classes:
            return [], [0], b""
        eng, arr, keep, counts, bufs = self._native_classes("group_values_packed", classes)
        want = [0, *accumulate(_engine.group_count(cnt, g) for cnt, g in zip(counts, groups))]
        total = sum(counts)
        weights, seed = self._weights(total)
        grp = (ctypes.c_uint64 * len(classes))(*groups)           # (a group of 0 is the native call's argument error)
        values = ctypes.create_string_buffer(64 * max(want[-1], 1))
        value_off = (ctypes.c_uint64 * (len(classes) + 1))()
        status = ctypes.create_string_buffer(max(total, 1))
        eng._ck(eng.lib.bpmi_rp_batch_group_values_mixed_dev(eng.ctx, len(classes), ctypes.cast(arr, ctypes.c_void_p), self.N, ctypes.cast(grp, ctypes.c_void_p), weights, seed,
                                                             self._d_gens.ptr, bufs[1].ptr, bufs[2].ptr, ctypes.cast(values, ctypes.c_void_p),
                                                             ctypes.cast(value_off, ctypes.c_void_p), ctypes.cast(status, ctypes.c_void_p)))
        del keep
        if list(value_off) != want:
            raise RuntimeError("bpmi_rp_batch_group_values_mixed_dev wrote the group offsets %r where %r were expected" % (list(value_off), want))
        raw = values.raw
        return [raw[64 * t: 64 * t + 64] for t in range(want[-1])], want, status.raw[:total]

    def _packed_items(self, items, classes, sel=None):
        """The packed form of the classes `classes` (what self.classes(items) returns) over items; sel: per class the positions inside
        its index list that take part (None: all)."""
        packed = []
        for c, (n, m, _, idx) in enumerate(classes):
            if sel is not None:
                idx = [idx[j] for j in sel[c]]
            packed.append((n, b"".join(P.to_le64() for i in idx for P in self._commitments(items[i][0])), [bytes(items[i][1]) for i in idx], None))
        return packed

    def group_values_wire(self, items, groups=None):
        """group_values_packed over items in any order: (values, value_off, status, index lists) -- the classes of self.classes(items),
        class c's index list saying which item each of its proofs is, so that global index first_c + j is item index_lists[c][j].
        groups: None = each class's default_group(m) over its prefix, an integer for every class, or a list with one per class.  Raises
        Exception("Proof invalid") only where classes() does: a proof whose size cannot be read."""
        items = list(items)
        if not items:
            return [], [0], b"", []
        classes = self.classes(items)
        grp = self.default_groups([(n, m) for n, m, _, _ in classes]) if groups is None else self._class_groups(groups, len(classes))
        values, value_off, status = self.group_values_packed(self._packed_items(items, classes), grp)
        return values, value_off, status, [idx for _, _, _, idx in classes]

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

    def locate_wire(self, items, group=0):
        """The sorted indices, in the CALLER's order, of every invalid proof of `items`; [] for a valid batch.  A proof whose size cannot
        be read, or does not fit this verifier, is invalid.
        group = 0 (the default): class by class through BatchRangeVerifier.locate_wire of the verifier over the class's prefix -- up to
        two native calls, uploads and preparations per class.
        group = None, an integer >= 1 or a list with one integer per class: the two levels of locate.locate_plan_groups over
        group_values_packed (bpmi_rp_batch_group_values_mixed_dev) -- level 1 is ONE call over every class with those group sizes (None:
        default_groups), level 2 ONE call with one proof per group over the unflagged proofs of the groups whose value is not the
        identity; a class with nothing selected is left out of that call.  A valid batch costs one native call, a rejected one two.  The
        indices are the same in every case.  Measured: tools/bench_rp_locate_mixed.py, DESIGN section 6s."""
        items = list(items)
        bad, sound = [], []
        for i, it in enumerate(items):
            try:
                self.classes([it])
                sound.append(i)
            except Exception:
                bad.append(i)
        if group is None or isinstance(group, (list, tuple)) or int(group) != 0:
            return sorted(bad + [sound[i] for i in self._locate_by_groups([items[i] for i in sound], group)])
        for n, m, _, idx in self.classes([items[i] for i in sound]):
            idx = [sound[j] for j in idx]
            Vs = [self._commitments(items[i][0]) for i in idx]
            found = self.prefix_verifier(n).locate_wire(Vs if m > 1 else [v[0] for v in Vs], [bytes(items[i][1]) for i in idx])
            bad += [idx[j] for j in found]
        return sorted(bad)

    def _locate_by_groups(self, items, group):
        """locate_wire's two-level plan over items whose classes can all be read: the indices into items of the invalid ones."""
        if not items:
            return []
        classes = self.classes(items)
        groups = self.default_groups([(n, m) for n, m, _, _ in classes]) if group is None else self._class_groups(group, len(classes))

        def group_values(sel, grp):
            if sel is None:
                return self.group_values_packed(self._packed_items(items, classes), grp)
            live = [c for c in range(len(classes)) if sel[c]]          # the native call refuses an empty class: it gets an empty range here
            values, off, status = self.group_values_packed(self._packed_items(items, [classes[c] for c in live], [sel[c] for c in live]), [grp[c] for c in live])
            ends = dict(zip(live, off[1:]))
            value_off = [0]
            for c in range(len(classes)):
                value_off.append(ends.get(c, value_off[-1]))
            return values, value_off, status

        flat = [i for _, _, _, idx in classes for i in idx]            # global (class-major) index -> index into items
        return [flat[i] for i in locate_plan_groups([len(idx) for _, _, _, idx in classes], groups, group_values)]
