"""Engine: one bpmi_ctx (one GPU, one stream) plus byte-level helpers.

This is the only module that talks to libbpmi.so.  Everything above it (the
reference-shaped Python call surface in pippenger/, utils/, innerproduct/,
rangeproofs/) goes through an Engine; nothing here or above computes EC or bulk
scalar arithmetic on the CPU.
"""
import ctypes
import os
import threading

from . import _native

Q = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
P_FIELD = 2**256 - 2**32 - 977
MAX_N = 1 << 26         # BPMI_MAX_N


class HostBuffer:
    """Page-locked host memory owned by an Engine (bpmi_host_alloc): `view` is a writable memoryview over it (recv_into it,
    slice-assign into it), `ptr` its address.  Uploads from it need no staging copy."""

    def __init__(self, engine, nbytes):
        self.engine = engine
        self.nbytes = nbytes
        p = ctypes.c_void_p()
        engine._ck(engine.lib.bpmi_host_alloc(engine.ctx, nbytes, ctypes.byref(p)))
        self.ptr = p.value
        self.view = memoryview((ctypes.c_char * nbytes).from_address(self.ptr)).cast("B")

    def __len__(self):
        return self.nbytes

    def free(self):
        if self.ptr:
            self.view.release()
            self.engine.lib.bpmi_host_free(self.engine.ctx, self.ptr)
            self.ptr = None


class EngineError(RuntimeError):
    pass


class DeviceBuffer:
    """hipMalloc'd bytes owned by an Engine."""

    def __init__(self, engine, nbytes):
        self.engine = engine
        self.nbytes = nbytes
        p = ctypes.c_void_p()
        engine._ck(engine.lib.bpmi_malloc(engine.ctx, nbytes, ctypes.byref(p)))
        self.ptr = p.value

    def upload(self, data, offset=0):
        assert offset + len(data) <= self.nbytes
        self.engine._ck(self.engine.lib.bpmi_upload(self.engine.ctx, self.ptr + offset, bytes(data), len(data)))
        return self

    def download(self, nbytes=None, offset=0):
        nbytes = self.nbytes - offset if nbytes is None else nbytes
        out = ctypes.create_string_buffer(nbytes)
        self.engine._ck(self.engine.lib.bpmi_download(self.engine.ctx, out, self.ptr + offset, nbytes))
        return out.raw

    def free(self):
        if self.ptr:
            self.engine.lib.bpmi_free(self.engine.ctx, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Engine:
    def __init__(self, device=None, stream=None):
        self.lib = _native.load()
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0")) % max(self.lib.bpmi_device_count(), 1)
        self.device = device
        self.ctx = self.lib.bpmi_ctx_create(device, stream)
        if not self.ctx:
            raise EngineError("bpmi_ctx_create failed: %s" % self.lib.bpmi_last_error(None).decode())
        # A/B experiments on code that creates its own engines (the bench's batches in flight): BPMI_OPTIONS="name=value,name=value"
        for kv in filter(None, os.environ.get("BPMI_OPTIONS", "").split(",")):
            name, _, value = kv.partition("=")
            self.set_option(name.strip(), int(value))

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.bpmi_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise EngineError("libbpmi error %d: %s" % (rc, self.lib.bpmi_last_error(self.ctx).decode()))

    def set_option(self, name, value):
        self._ck(self.lib.bpmi_set_option(self.ctx, name.encode(), int(value)))

    def sync(self):
        self._ck(self.lib.bpmi_sync(self.ctx))

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def host_alloc(self, nbytes):
        return HostBuffer(self, nbytes)

    def upload(self, data):
        return DeviceBuffer(self, max(len(data), 16)).upload(data)

    # ---- byte-level operations (wire format of include/bpmi.h) ----
    def msm_bytes(self, pts, scalars, n):
        out = ctypes.create_string_buffer(64)
        self._ck(self.lib.bpmi_msm(self.ctx, pts, scalars, n, out))
        return out.raw

    def msm2_bytes(self, pts0, scalars0, n0, pts1, scalars1, n1):
        """Two independent MSMs overlapped on the engine's two lanes -> (64 bytes, 64 bytes)."""
        o0, o1 = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
        self._ck(self.lib.bpmi_msm2(self.ctx, pts0, scalars0, n0, o0, pts1, scalars1, n1, o1))
        return o0.raw, o1.raw

    def msm_dev(self, d_pts, d_scalars, n):
        out = ctypes.create_string_buffer(64)
        self._ck(self.lib.bpmi_msm_dev(self.ctx, _ptr(d_pts), _ptr(d_scalars), n, out))
        return out.raw

    def msm_dev_enqueue(self, slot, d_pts, d_scalars, n):
        """Queue one MSM (device pointers, n <= 2^23) in pending slot 0 or 1 and return at once."""
        self._ck(self.lib.bpmi_msm_dev_enqueue(self.ctx, slot, _ptr(d_pts), _ptr(d_scalars), n))

    def msm_finish(self, slot):
        """Wait for the MSM of `slot` only and return its 64-byte result."""
        out = ctypes.create_string_buffer(64)
        self._ck(self.lib.bpmi_msm_finish(self.ctx, slot, out))
        return out.raw

    def msm_batch_dev(self, d_pts, ns, d_scalars, n_vec, d_out=None):
        """n_vec MSMs over ONE shared point set (bpmi_msm_batch_dev): d_pts / ns / d_scalars name 1 .. 3 segments -- ns[s] points each,
        d_scalars[s] a row-major matrix of n_vec rows of ns[s] scalars.  Returns the n_vec x 64 result bytes; with d_out (device memory,
        n_vec x 64 bytes) the work is only queued (bpmi_msm_batch_dev_enqueue), None is returned and d_out is read after sync()."""
        nseg = len(ns)
        if not (len(d_pts) == len(d_scalars) == nseg):
            raise ValueError("d_pts, ns and d_scalars name the same segments")
        P = (ctypes.c_void_p * nseg)(*[_ptr(p) if p is not None else None for p in d_pts])
        S = (ctypes.c_void_p * nseg)(*[_ptr(s) if s is not None else None for s in d_scalars])
        N = (ctypes.c_uint64 * nseg)(*ns)
        if d_out is not None:
            self._ck(self.lib.bpmi_msm_batch_dev_enqueue(self.ctx, nseg, P, N, S, n_vec, _ptr(d_out)))
            return None
        out = ctypes.create_string_buffer(max(64 * n_vec, 1))
        self._ck(self.lib.bpmi_msm_batch_dev(self.ctx, nseg, P, N, S, n_vec, out))
        return out.raw[:64 * n_vec]

    def msm_batch_bytes(self, pts, scalars, n, n_vec):
        """The same from host bytes, one segment (bpmi_msm_batch): pts n x 64 bytes, scalars n_vec rows of n x 32 bytes."""
        out = ctypes.create_string_buffer(max(64 * n_vec, 1))
        self._ck(self.lib.bpmi_msm_batch(self.ctx, pts, n, scalars, n_vec, out))
        return out.raw[:64 * n_vec]

    def fixed_base_create(self, pts, n, window_bits=0, rows=0):
        """A FixedBase over n points (bpmi_fixed_base_create[_dev]): `pts` is n x 64 host bytes, or device memory (a DeviceBuffer, a tensor,
        an address).  window_bits / rows: 0 = automatic, else 10 .. 16 / 1 .. W; the points are copied."""
        h = ctypes.c_void_p()
        if isinstance(pts, (bytes, bytearray)):
            self._ck(self.lib.bpmi_fixed_base_create(self.ctx, bytes(pts), n, window_bits, rows, ctypes.byref(h)))
        else:
            self._ck(self.lib.bpmi_fixed_base_create_dev(self.ctx, _ptr(pts), n, window_bits, rows, ctypes.byref(h)))
        return FixedBase(self, h.value)

    def msm_geometry(self, n, pipelined=False):
        """What an MSM of n pairs runs as under the current options (bpmi_msm_geometry): a dict with the kernel family, window bits,
        windows (and how many are one bit wider), buckets, chunk length, slices and pairs per slice.  No GPU work."""
        g = (ctypes.c_uint32 * 8)()
        self._ck(self.lib.bpmi_msm_geometry(self.ctx, n, 1 if pipelined else 0, g))
        return {"kernel": ("pipeline", "small", "mid")[g[0]] if n else None, "window_bits": g[1], "windows": g[2], "wide_windows": g[3],
                "buckets": g[4], "chunk": g[5], "slices": g[6], "pairs_per_slice": g[7]}

    def msm_runs_state(self, lane=0):
        """Which accumulation the last bucket-pipeline MSM of `lane` ran (bpmi_debug_msm_runs; tests): a dict with `planned` (the accumulation
        by runs was planned), `long_run` (the device found a run over the cap: the chunked accumulation did the work) and `runs`."""
        st = (ctypes.c_uint32 * 3)()
        self._ck(self.lib.bpmi_debug_msm_runs(self.ctx, lane, st))
        return {"planned": bool(st[0]), "long_run": bool(st[1]), "runs": st[2]}

    def ec_mul_batch_bytes(self, pts, scalars, n):
        out = ctypes.create_string_buffer(64 * n)
        self._ck(self.lib.bpmi_ec_mul_batch(self.ctx, pts, scalars, n, out))
        return out.raw

    def ec_lincomb2_batch_bytes(self, p1, p2, k1, k2, n):
        out = ctypes.create_string_buffer(64 * n)
        self._ck(self.lib.bpmi_ec_lincomb2_batch(self.ctx, p1, p2, k1, k2, n, out))
        return out.raw

    def ec_sum_bytes(self, pts, n):
        out = ctypes.create_string_buffer(64)
        self._ck(self.lib.bpmi_ec_sum(self.ctx, pts, n, out))
        return out.raw

    def ec_sum_dev(self, d_pts, n):
        out = ctypes.create_string_buffer(64)
        self._ck(self.lib.bpmi_ec_sum_dev(self.ctx, _ptr(d_pts), n, out))
        return out.raw

    def ec_decompress_batch_bytes(self, comp, n):
        """n x 33-byte SEC1 compressed points -> (n x 64-byte wire points, n validity flags)."""
        out = ctypes.create_string_buffer(64 * n)
        ok = ctypes.create_string_buffer(max(n, 1))
        self._ck(self.lib.bpmi_ec_decompress_batch(self.ctx, comp, n, out, ok))
        return out.raw, ok.raw[:n]

    # ---- bulk hash to the curve (bpmi_ec_hash_*): the reference's elliptic_hash for many messages at once ----
    @staticmethod
    def _hash_buffers(n, with_tries, points=True):
        n = n if 0 < n <= MAX_N else 0               # (a count the library refuses: nothing is allocated for it here either)
        return (ctypes.create_string_buffer(max(64 * n, 1)) if points else None), (ctypes.create_string_buffer(max(n, 1)) if with_tries else None)

    def _hash_result(self, n, out, tries):
        if tries is None:
            return out
        return out, tries.raw[:n]

    def ec_hash_batch_bytes(self, msgs, max_tries=0, with_tries=False, offsets=None):
        """elliptic_hash of every message -> n x 64-byte wire points.  msgs: a list of byte strings, or with `offsets` (n + 1
        numbers) the packed bytes they index.  with_tries: also the n counters that succeeded (0: no point within max_tries, the
        point is then 64 zero bytes); without it such a message raises EngineError."""
        packed, off, n = _pack_messages(msgs, offsets)
        out, tries = self._hash_buffers(n, with_tries)
        self._ck(self.lib.bpmi_ec_hash_batch(self.ctx, packed, off, n, max_tries, out, tries))
        return self._hash_result(n, out.raw[:64 * n], tries)

    def ec_hash_batch_dev(self, msgs, max_tries=0, with_tries=False, offsets=None, d_out=None):
        """The same with the points left in device memory: `d_out` (n x 64 bytes) is filled, or a new DeviceBuffer returned."""
        packed, off, n = _pack_messages(msgs, offsets)
        d_out = self.alloc(max(64 * n, 16) if n <= MAX_N else 16) if d_out is None else d_out
        _, tries = self._hash_buffers(n, with_tries, points=False)
        self._ck(self.lib.bpmi_ec_hash_batch_dev(self.ctx, packed, off, n, max_tries, _ptr(d_out), tries))
        return self._hash_result(n, d_out, tries)

    def ec_hash_range_bytes(self, tail, lo, hi, max_tries=0, with_tries=False):
        """elliptic_hash(str(i) || tail) for i in [lo, hi) -> (hi - lo) x 64-byte wire points (and the counters, as above)."""
        n = max(hi - lo, 0)
        out, tries = self._hash_buffers(n, with_tries)
        self._ck(self.lib.bpmi_ec_hash_range(self.ctx, bytes(tail), len(tail), lo, hi, max_tries, out, tries))
        return self._hash_result(n, out.raw[:64 * n], tries)

    def ec_hash_range_dev(self, tail, lo, hi, max_tries=0, with_tries=False, d_out=None):
        """The same with the points left in device memory, ready to be the generators of an MSM or of an inner-product argument."""
        n = max(hi - lo, 0)
        d_out = self.alloc(max(64 * n, 16) if n <= MAX_N else 16) if d_out is None else d_out
        _, tries = self._hash_buffers(n, with_tries, points=False)
        self._ck(self.lib.bpmi_ec_hash_range_dev(self.ctx, bytes(tail), len(tail), lo, hi, max_tries, _ptr(d_out), tries))
        return self._hash_result(n, d_out, tries)

    def sc_dot_bytes(self, a, b, n):
        out = ctypes.create_string_buffer(32)
        self._ck(self.lib.bpmi_sc_dot(self.ctx, a, b, n, out))
        return out.raw

    def sc_fold_bytes(self, lo, hi, x, y, n):
        out = ctypes.create_string_buffer(32 * n)
        self._ck(self.lib.bpmi_sc_fold(self.ctx, lo, hi, x, y, n, out))
        return out.raw

    def sc_svector_bytes(self, xs, xinvs, k, a, b, scale=None):
        """(sa, sb) of bpmi_sc_svector as packed bytes, 2^k scalars each."""
        n = 1 << k
        sa, sb = ctypes.create_string_buffer(32 * n), ctypes.create_string_buffer(32 * n)
        self._ck(self.lib.bpmi_sc_svector(self.ctx, xs, xinvs, k, sc_bytes(a), sc_bytes(b), scale, sa, sb))
        return sa.raw, sb.raw

    def ipa_verify_dev(self, d_g, d_h, n, xs, xinvs, a, b, extra_pts, extra_scalars, n_extra, d_hscale=None):
        """The 64-byte value of Verifier2's combined check over device-resident generators (identity = accept)."""
        out = ctypes.create_string_buffer(64)
        k = n.bit_length() - 1
        self._ck(self.lib.bpmi_ipa_verify_dev(self.ctx, _ptr(d_g), _ptr(d_h), None if d_hscale is None else _ptr(d_hscale), n, xs, xinvs, k,
                                              sc_bytes(a), sc_bytes(b), extra_pts, extra_scalars, n_extra, out))
        return out.raw

    def sc_svector_sum_bytes(self, k, n_proofs, xs, xinvs, a, b, weights, scale=None):
        """(SA, SB) of bpmi_sc_svector_sum as packed bytes, 2^k scalars each: the weighted sums of n_proofs s-vectors.  xs, xinvs:
        n_proofs x k packed scalars; a, b, weights: n_proofs packed scalars each; scale: 2^k packed scalars or None."""
        n = 1 << k
        sa, sb = ctypes.create_string_buffer(32 * n), ctypes.create_string_buffer(32 * n)
        self._ck(self.lib.bpmi_sc_svector_sum(self.ctx, k, n_proofs, xs, xinvs, a, b, weights, scale, sa, sb))
        return sa.raw, sb.raw

    def ipa_verify_batch_dev(self, d_g, d_h, n, n_proofs, xs, xinvs, a, b, weights, extra_pts, extra_scalars, n_extra, d_hscale=None):
        """The 64-byte value of a batch of Verifier2 checks over device-resident generators under the given weights (identity =
        every proof accepted).  Packed bytes throughout; the extra scalars arrive multiplied by their proof's weight."""
        out = ctypes.create_string_buffer(64)
        k = n.bit_length() - 1
        self._ck(self.lib.bpmi_ipa_verify_batch_dev(self.ctx, _ptr(d_g), _ptr(d_h), None if d_hscale is None else _ptr(d_hscale), n, n_proofs,
                                                    xs, xinvs, k, a, b, weights, extra_pts, extra_scalars, n_extra, out))
        return out.raw

    def sc_svector_sum_mixed_bytes(self, n_gens, ks, xs, xinvs, a, b, weights, scale=None):
        """(SA, SB) of bpmi_sc_svector_sum_mixed as packed bytes, n_top = 2^max(ks) scalars each: the weighted sums of the s-vectors of
        proofs of different lengths 2^ks[p] over the prefixes of n_gens generators.  xs, xinvs: every proof's ks[p] packed challenges,
        proof after proof; a, b, weights: one packed scalar per proof; scale: n_gens packed scalars or None."""
        n = 1 << min(max(ks, default=0), 22)           # (a longer proof is refused by the call)
        sa, sb, n_top = ctypes.create_string_buffer(32 * n), ctypes.create_string_buffer(32 * n), ctypes.c_uint64(0)
        self._ck(self.lib.bpmi_sc_svector_sum_mixed(self.ctx, n_gens, len(ks), (ctypes.c_uint32 * max(len(ks), 1))(*ks), xs, xinvs, a, b, weights, scale,
                                                    sa, sb, ctypes.byref(n_top)))
        return sa.raw[:32 * n_top.value], sb.raw[:32 * n_top.value]

    def ipa_verify_batch_mixed_dev(self, d_g, d_h, n_gens, ks, xs, xinvs, a, b, weights, extra_pts, extra_scalars, n_extra, d_hscale=None):
        """The 64-byte value of a batch of Verifier2 checks of different lengths 2^ks[p] over the prefixes of n_gens device-resident
        generators under the given weights (identity = every proof accepted); argument forms as ipa_verify_batch_dev."""
        out = ctypes.create_string_buffer(64)
        self._ck(self.lib.bpmi_ipa_verify_batch_mixed_dev(self.ctx, _ptr(d_g), _ptr(d_h), None if d_hscale is None else _ptr(d_hscale), n_gens, len(ks),
                                                          (ctypes.c_uint32 * max(len(ks), 1))(*ks), xs, xinvs, a, b, weights, extra_pts, extra_scalars,
                                                          n_extra, out))
        return out.raw

    # ---- packed inner-product proofs (what bpmi_ipa_prove_batch writes) ----
    def ipa_batch_prepare_dev(self, k, protocol, count, ab, xs, lr, transcripts, starts, u, P, c=None, head=None, weights=None, seed=None):
        """(records, extra_pts, extra_scalars, status) of bpmi_ipa_batch_prepare_dev as bytes: the per-proof preparation of the packed
        batch verifier by the device kernels; argument forms as ipa_batch_prepare_host."""
        pairs = count * (2 * k + (4 if protocol == 1 else 2))
        d_rec, d_pts, d_sc = self.alloc(max((64 * k + 96) * count, 16)), self.alloc(max(64 * pairs, 16)), self.alloc(max(32 * pairs, 16))
        status = ctypes.create_string_buffer(max(count, 1))
        try:
            self._ck(self.lib.bpmi_ipa_batch_prepare_dev(self.ctx, k, protocol, count, *packed_proof_args(count, ab, xs, lr, transcripts, starts, u, P, c, head),
                                                         weights, seed, d_rec.ptr, d_pts.ptr, d_sc.ptr, ctypes.cast(status, ctypes.c_void_p)))
            return d_rec.download((64 * k + 96) * count), d_pts.download(64 * pairs), d_sc.download(32 * pairs), status.raw[:count]
        finally:
            for d in (d_rec, d_pts, d_sc):
                d.free()

    def ipa_verify_batch_packed_dev(self, d_g, d_h, n, protocol, count, ab, xs, lr, transcripts, starts, u, P, c=None, head=None, weights=None, seed=None,
                                    d_hscale=None):
        """(out, status) of bpmi_ipa_verify_batch_packed_dev: the 64-byte value of the weighted combination over the unflagged proofs
        (identity = all of them verify) and one status byte per proof (0 = passed the byte-level and on-curve checks)."""
        out, status = ctypes.create_string_buffer(64), ctypes.create_string_buffer(max(count, 1))
        self._ck(self.lib.bpmi_ipa_verify_batch_packed_dev(self.ctx, _ptr(d_g), _ptr(d_h), None if d_hscale is None else _ptr(d_hscale), n, protocol, count,
                                                           *packed_proof_args(count, ab, xs, lr, transcripts, starts, u, P, c, head), weights, seed,
                                                           ctypes.cast(out, ctypes.c_void_p), ctypes.cast(status, ctypes.c_void_p)))
        return out.raw, status.raw[:count]

    # ---- inner-product proofs in the wire format BPIP2 (innerproduct/codec.py) ----
    def ipa_wire_expand_dev(self, k, blobs, off, protocol=2):
        """(ab, xs, lr, transcripts, starts, status) of bpmi_ipa_wire_expand_dev: the packed arrays a batch of blobs (joined bytes and
        len(off) - 1 proofs) stands for, rebuilt by the device kernels and downloaded; the bytes of codec.packed_from_wire."""
        count = len(off) - 1
        if count <= 0:
            return b"", b"", b"", [], [], b""
        offs = (ctypes.c_uint64 * (count + 1))(*off)
        cap = max(sum(max(off[i + 1] - off[i] - (78 + 98 * k), 0) for i in range(count)) + 169 * k * count, 1)
        ab, xs, lr = ctypes.create_string_buffer(64 * count), ctypes.create_string_buffer(max(32 * k * count, 1)), ctypes.create_string_buffer(max(128 * k * count, 1))
        tr, tr_off, start, status = ctypes.create_string_buffer(cap), (ctypes.c_uint64 * (count + 1))(), (ctypes.c_uint32 * count)(), ctypes.create_string_buffer(count)
        self._ck(self.lib.bpmi_ipa_wire_expand_dev(self.ctx, k, protocol, count, bytes(blobs), offs, ab, xs, lr, tr, cap, tr_off, start, status))
        raw = tr.raw
        return (ab.raw, xs.raw[: 32 * k * count], lr.raw[: 128 * k * count], [raw[tr_off[i]: tr_off[i + 1]] for i in range(count)], list(start),
                status.raw[:count])

    def ipa_verify_batch_wire_dev(self, d_g, d_h, n, count, blobs, off, u, P, weights=None, seed=None, d_hscale=None, protocol=2):
        """(out, status) of bpmi_ipa_verify_batch_wire_dev: ipa_verify_batch_packed_dev over the proofs the blobs stand for, expanded in
        device memory.  blobs: joined bytes; off: count + 1 offsets (a list or a ctypes array of uint64); u, P: 64 bytes per proof."""
        out, status = ctypes.create_string_buffer(64), ctypes.create_string_buffer(max(count, 1))
        offs = off if isinstance(off, ctypes.Array) else (ctypes.c_uint64 * (count + 1))(*off)
        self._ck(self.lib.bpmi_ipa_verify_batch_wire_dev(self.ctx, _ptr(d_g), _ptr(d_h), None if d_hscale is None else _ptr(d_hscale), n, protocol, count,
                                                         blobs if isinstance(blobs, bytes) else bytes(blobs), offs, u, P, weights, seed, ctypes.cast(out, ctypes.c_void_p), ctypes.cast(status, ctypes.c_void_p)))
        return out.raw, status.raw[:count]

    def ipa_group_values_packed_dev(self, d_g, d_h, n, protocol, count, ab, xs, lr, transcripts, starts, u, P, c=None, head=None, weights=None, seed=None,
                                    d_hscale=None, group=1):
        """(values, status) of bpmi_ipa_group_values_packed_dev: values[t] = the 64-byte value of the weighted combination over the
        unflagged proofs of [t group, (t + 1) group) (identity = all of them verify) -- what ipa_verify_batch_packed_dev returns for that
        sub-batch under the same weights -- and one status byte per proof.  One preparation and one launch of the groups' MSMs."""
        ngroups = group_count(count, group)
        values, status = ctypes.create_string_buffer(max(64 * ngroups, 1)), ctypes.create_string_buffer(max(count, 1))
        self._ck(self.lib.bpmi_ipa_group_values_packed_dev(self.ctx, _ptr(d_g), _ptr(d_h), None if d_hscale is None else _ptr(d_hscale), n, protocol, count,
                                                           *packed_proof_args(count, ab, xs, lr, transcripts, starts, u, P, c, head), weights, seed, group,
                                                           ctypes.cast(values, ctypes.c_void_p), ctypes.cast(status, ctypes.c_void_p)))
        raw = values.raw
        return [raw[64 * t: 64 * t + 64] for t in range(ngroups)], status.raw[:count]

    # ---- packed inner-product proofs of different lengths: a list of classes (bpmi_ipa_packed_class) ----
    def ipa_batch_prepare_mixed_dev(self, K, protocol, classes, weights=None, seed=None):
        """(records, rec_byte_off, extra_pts, extra_scalars, status) of bpmi_ipa_batch_prepare_mixed_dev: the preparation of a mixed packed
        batch by the device kernels; argument forms as ipa_batch_prepare_mixed_host."""
        arr, keep, total, rec_bytes, pairs = packed_class_array(protocol, classes)
        d_rec, d_pts, d_sc = self.alloc(max(rec_bytes, 16)), self.alloc(max(64 * pairs, 16)), self.alloc(max(32 * pairs, 16))
        status, offs = ctypes.create_string_buffer(max(total, 1)), (ctypes.c_uint64 * max(len(classes), 1))()
        try:
            self._ck(self.lib.bpmi_ipa_batch_prepare_mixed_dev(self.ctx, K, protocol, len(classes), ctypes.addressof(arr), weights, seed, d_rec.ptr,
                                                               ctypes.addressof(offs), d_pts.ptr, d_sc.ptr, ctypes.cast(status, ctypes.c_void_p)))
            return d_rec.download(rec_bytes), list(offs)[:len(classes)], d_pts.download(64 * pairs), d_sc.download(32 * pairs), status.raw[:total]
        finally:
            del keep
            for d in (d_rec, d_pts, d_sc):
                d.free()

    def ipa_verify_batch_packed_mixed_dev(self, d_g, d_h, n_gens, protocol, classes, weights=None, seed=None, d_hscale=None):
        """(out, status) of bpmi_ipa_verify_batch_packed_mixed_dev: the 64-byte value of the weighted combination over the unflagged
        proofs of every class (identity = all of them verify) and one status byte per proof, class-major.  classes: a list of
        (k, count, ab, xs, lr, transcripts, starts, u, P, c, head) -- per class the arguments of ipa_verify_batch_packed_dev."""
        arr, keep, total, _, _ = packed_class_array(protocol, classes)
        out, status = ctypes.create_string_buffer(64), ctypes.create_string_buffer(max(total, 1))
        self._ck(self.lib.bpmi_ipa_verify_batch_packed_mixed_dev(self.ctx, _ptr(d_g), _ptr(d_h), None if d_hscale is None else _ptr(d_hscale), n_gens, protocol,
                                                                 len(classes), ctypes.addressof(arr), weights, seed, ctypes.cast(out, ctypes.c_void_p),
                                                                 ctypes.cast(status, ctypes.c_void_p)))
        del keep
        return out.raw, status.raw[:total]

    def ipa_group_values_packed_mixed_dev(self, d_g, d_h, n_gens, protocol, classes, groups, weights=None, seed=None, d_hscale=None):
        """(values, value_off, status) of bpmi_ipa_group_values_packed_mixed_dev.  classes: as ipa_verify_batch_packed_mixed_dev; groups: one
        group size per class.  values: one 64-byte string per group, class-major -- class c owns values[value_off[c]: value_off[c + 1]],
        groups of min(groups[c], count_c) consecutive proofs, the last one possibly short; values[t] is the weighted combination over
        the unflagged proofs of group t (identity = all of them verify).  status: one byte per proof, class-major."""
        if len(groups) != len(classes):
            raise ValueError("one group size per class")
        arr, keep, total, _, _ = packed_class_array(protocol, classes)
        ngroups = sum(group_count(cl[1], g) for cl, g in zip(classes, groups))
        grp = (ctypes.c_uint64 * max(len(classes), 1))(*[int(g) for g in groups])
        offs = (ctypes.c_uint64 * (len(classes) + 1))()
        values, status = ctypes.create_string_buffer(max(64 * ngroups, 1)), ctypes.create_string_buffer(max(total, 1))
        self._ck(self.lib.bpmi_ipa_group_values_packed_mixed_dev(self.ctx, _ptr(d_g), _ptr(d_h), None if d_hscale is None else _ptr(d_hscale), n_gens, protocol,
                                                                 len(classes), ctypes.addressof(arr), ctypes.addressof(grp), weights, seed,
                                                                 ctypes.cast(values, ctypes.c_void_p), ctypes.addressof(offs), ctypes.cast(status, ctypes.c_void_p)))
        del keep
        raw, offs = values.raw, list(offs)
        if offs[-1] != ngroups:
            raise RuntimeError("bpmi_ipa_group_values_packed_mixed_dev wrote %d groups where %d were expected" % (offs[-1], ngroups))
        return [raw[64 * t: 64 * t + 64] for t in range(ngroups)], offs, status.raw[:total]

    def ipap_t_budget(self, nbytes):
        """bpmi_debug_ipap_t_budget (tests): the transposition budget of the mixed packed calls and of ipa_group_values_packed_dev on this engine; 0 restores
        the default."""
        self._ck(self.lib.bpmi_debug_ipap_t_budget(self.ctx, nbytes))

    # ---- IPA prover state ----
    def ipa_create(self, g, h, a, b, n, u, h_scale=None):
        st = ctypes.c_void_p()
        if h_scale is None:
            self._ck(self.lib.bpmi_ipa_create(self.ctx, g, h, a, b, n, u, ctypes.byref(st)))
        else:
            self._ck(self.lib.bpmi_ipa_create_scaled(self.ctx, g, h, a, b, n, u, h_scale, ctypes.byref(st)))
        return IpaState(self, st.value)

    def ipa_create_dev(self, d_g, d_h, d_a, d_b, n, u):
        st = ctypes.c_void_p()
        self._ck(self.lib.bpmi_ipa_create_dev(self.ctx, _ptr(d_g), _ptr(d_h), _ptr(d_a), _ptr(d_b), n, u, ctypes.byref(st)))
        return IpaState(self, st.value)

    # ---- profiling ----
    def profile(self, enable=True):
        """True / 1: HIP events around every stage; 2: around the dominant stage only; False: off."""
        self._ck(self.lib.bpmi_profile(self.ctx, int(enable)))

    def profile_reset(self):
        self._ck(self.lib.bpmi_profile_reset(self.ctx))

    def profile_read(self):
        ms = (ctypes.c_double * _native.NSTAGES)()
        calls = (ctypes.c_uint64 * _native.NSTAGES)()
        self._ck(self.lib.bpmi_profile_read(self.ctx, ms, calls))
        return {self.lib.bpmi_profile_stage_name(i).decode(): (ms[i], calls[i]) for i in range(_native.NSTAGES)}


class FixedBase:
    """A point set and the table of its multiples on the device (bpmi_fixed_base, include/bpmi.h): MSMs over the first n_scalars of its
    points, through the engine's lanes and pending slots like msm_dev / msm_dev_enqueue.  Close it before its engine."""

    def __init__(self, engine, handle):
        self.engine = engine
        self.handle = handle

    @property
    def info(self):
        v = (ctypes.c_uint64 * 8)()
        self.engine._ck(self.engine.lib.bpmi_fixed_base_info(self.handle, v))
        return {"n": v[0], "window_bits": v[1], "windows": v[2], "rows": v[3], "virtual_windows": v[4], "table_bytes": v[5], "build_us": v[6]}

    def table_bytes(self, row, first, count):
        out = ctypes.create_string_buffer(max(64 * count, 1))
        self.engine._ck(self.engine.lib.bpmi_fixed_base_table(self.handle, row, first, count, out))
        return out.raw[:64 * count]

    def msm_bytes(self, scalars, n_scalars):
        out = ctypes.create_string_buffer(64)
        self.engine._ck(self.engine.lib.bpmi_msm_fixed(self.handle, scalars, n_scalars, out))
        return out.raw

    def msm_dev(self, d_scalars, n_scalars):
        out = ctypes.create_string_buffer(64)
        self.engine._ck(self.engine.lib.bpmi_msm_fixed_dev(self.handle, _ptr(d_scalars) if n_scalars else None, n_scalars, out))
        return out.raw

    def msm_dev_enqueue(self, slot, d_scalars, n_scalars):
        """Queue one MSM in pending slot `slot`; Engine.msm_finish(slot) returns its result."""
        self.engine._ck(self.engine.lib.bpmi_msm_fixed_dev_enqueue(self.handle, slot, _ptr(d_scalars) if n_scalars else None, n_scalars))

    def close(self):
        if self.handle and getattr(self.engine, "ctx", None):
            self.engine.lib.bpmi_fixed_base_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IpaState:
    """One FastNIProver2 run on the device, split at the Fiat-Shamir edge."""

    def __init__(self, engine, handle):
        self.engine = engine
        self.handle = handle

    def __len__(self):
        return self.engine.lib.bpmi_ipa_len(self.handle)

    def round_LR(self):
        L = ctypes.create_string_buffer(64)
        R = ctypes.create_string_buffer(64)
        self.engine._ck(self.engine.lib.bpmi_ipa_round_LR(self.handle, L, R))
        return L.raw, R.raw

    def fold(self, x, xinv):
        self.engine._ck(self.engine.lib.bpmi_ipa_fold(self.handle, sc_bytes(x), sc_bytes(xinv)))

    def prove_rounds(self, digest):
        """Every remaining round in one native call (bpmi_ipa_prove_rounds): the transcript `digest` so far ->
        (transcript after the last round, [x as int], [L as 64 bytes], [R as 64 bytes])."""
        k = max(1, len(self).bit_length())
        cap = len(digest) + 256 * k
        out, out_len, rounds = ctypes.create_string_buffer(cap), ctypes.c_uint64(0), ctypes.c_uint32(0)
        xs, Ls, Rs = ctypes.create_string_buffer(32 * k), ctypes.create_string_buffer(64 * k), ctypes.create_string_buffer(64 * k)
        self.engine._ck(self.engine.lib.bpmi_ipa_prove_rounds(self.handle, digest, len(digest), out, cap, ctypes.byref(out_len), xs, Ls, Rs, k,
                                                              ctypes.byref(rounds)))
        r = rounds.value
        return (out.raw[:out_len.value], [int.from_bytes(xs.raw[32 * i: 32 * i + 32], "little") for i in range(r)],
                [Ls.raw[64 * i: 64 * i + 64] for i in range(r)], [Rs.raw[64 * i: 64 * i + 64] for i in range(r)])

    def finish(self):
        a = ctypes.create_string_buffer(32)
        b = ctypes.create_string_buffer(32)
        self.engine._ck(self.engine.lib.bpmi_ipa_finish(self.handle, a, b))
        return int.from_bytes(a.raw, "little"), int.from_bytes(b.raw, "little")

    def export(self):
        """(g, h, a, b) of the current round as packed bytes: len(self) points / scalars each."""
        m = len(self)
        g, h = ctypes.create_string_buffer(64 * m), ctypes.create_string_buffer(64 * m)
        a, b = ctypes.create_string_buffer(32 * m), ctypes.create_string_buffer(32 * m)
        self.engine._ck(self.engine.lib.bpmi_ipa_export(self.handle, g, h, a, b))
        return g.raw, h.raw, a.raw, b.raw

    def close(self):
        if self.handle:
            self.engine.lib.bpmi_ipa_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _ptr(x):
    if isinstance(x, DeviceBuffer):
        return x.ptr
    if hasattr(x, "data_ptr"):  # torch tensor on the engine's device
        return x.data_ptr()
    return int(x)


def _pack_messages(msgs, offsets):
    """(packed bytes, n + 1 offsets as a C array, n) of a list of byte strings; `offsets` given: msgs is the packed bytes already."""
    if offsets is None:
        offsets = [0]
        for m in msgs:
            offsets.append(offsets[-1] + len(m))
        msgs = b"".join(msgs)
    n = len(offsets) - 1
    return bytes(msgs), (ctypes.c_uint64 * (n + 1))(*offsets), n


def sc_bytes(k):
    return (int(k) % Q).to_bytes(32, "little")


def group_count(count, group):
    """The groups of min(group, count) consecutive proofs that `count` proofs make, the last one possibly short (none for no proof):
    the clamp of the native group calls.  (group < 1 counts as 1 here; it is the native call's argument error.)"""
    g = min(max(int(group), 1), count)
    return (count + g - 1) // g if count else 0


def packed_proof_args(count, ab, xs, lr, transcripts, starts, u, P, c=None, head=None):
    """The packed-proof arguments of the bpmi_ipa_batch_prepare family (include/bpmi.h), in its order: ab, xs, LR, transcripts,
    tr_off, start, u, P, c, head.  transcripts: a list of `count` byte strings, or (joined bytes, count + 1 offsets); starts: None
    or `count` integers; empty xs / lr / c / head go as NULL.  The C arrays are kept alive by the returned tuple."""
    if isinstance(transcripts, tuple):
        joined, offs = transcripts
        tr_off = offs if isinstance(offs, ctypes.Array) else (ctypes.c_uint64 * len(offs))(*offs)
        joined = bytes(joined)
    else:
        joined, tr_off, _ = _pack_messages(list(transcripts), None)
    if len(tr_off) != count + 1:
        raise ValueError("one transcript per proof")
    start = None if starts is None else (ctypes.c_uint32 * count)(*starts)
    opt = lambda b: bytes(b) if b else None
    return (bytes(ab), opt(xs), opt(lr), joined, tr_off, start, bytes(u), bytes(P), opt(c), opt(head))


def ipa_batch_prepare_host(k, protocol, count, ab, xs, lr, transcripts, starts, u, P, c=None, head=None, weights=None, seed=None, threads=4):
    """(records, extra_pts, extra_scalars, status) of bpmi_ipa_batch_prepare as bytes: the per-proof preparation of the packed batch
    verifier in native HOST code (no GPU, no Engine).  Argument forms: packed_proof_args; weights: packed scalars (1 per proof under
    Protocol 2, 3 under Protocol 1) or None with a 32-byte seed."""
    lib = _native.load()
    pairs = count * (2 * k + (4 if protocol == 1 else 2))
    rec, pts, sc = (ctypes.create_string_buffer(max(nb, 1)) for nb in ((64 * k + 96) * count, 64 * pairs, 32 * pairs))
    status = ctypes.create_string_buffer(max(count, 1))
    vp = lambda b: ctypes.cast(b, ctypes.c_void_p)
    rc = lib.bpmi_ipa_batch_prepare(k, protocol, count, *packed_proof_args(count, ab, xs, lr, transcripts, starts, u, P, c, head), weights, seed, threads,
                                    vp(rec), vp(pts), vp(sc), vp(status))
    if rc != 0:
        raise EngineError("libbpmi error %d: %s" % (rc, lib.bpmi_last_error(None).decode()))
    return rec.raw[: (64 * k + 96) * count], pts.raw[: 64 * pairs], sc.raw[: 32 * pairs], status.raw[:count]


def packed_class_array(protocol, classes):
    """(array of IpaPackedClass, the objects its addresses point into, proofs, record bytes, extra pairs) of a list of classes
    (k, count, ab, xs, lr, transcripts, starts, u, P, c, head): per class the arguments of packed_proof_args behind its k.  A class
    with count = 0 keeps NULL pointers."""
    arr, keep = (_native.IpaPackedClass * max(len(classes), 1))(), []

    def addr(x):
        if x is None:
            return None
        if isinstance(x, ctypes.Array):
            keep.append(x)
            return ctypes.addressof(x)
        p = ctypes.c_char_p(x)
        keep.append((x, p))
        return ctypes.cast(p, ctypes.c_void_p).value
    total = rec_bytes = pairs = 0
    for i, (k, count, *rest) in enumerate(classes):
        arr[i].k, arr[i].n_proofs = k, count
        if not count:
            continue
        for name, v in zip(("ab", "xs", "LR", "transcripts", "tr_off", "start", "u", "P", "c", "head"), packed_proof_args(count, *rest)):
            setattr(arr[i], name, addr(v))
        total, rec_bytes, pairs = total + count, rec_bytes + (64 * k + 96) * count, pairs + count * (2 * k + (4 if protocol == 1 else 2))
    return arr, keep, total, rec_bytes, pairs


def ipa_batch_prepare_mixed_host(K, protocol, classes, weights=None, seed=None, threads=4):
    """(records, rec_byte_off, extra_pts, extra_scalars, status) of bpmi_ipa_batch_prepare_mixed as bytes: the preparation of a mixed packed
    batch in native HOST code (no GPU, no Engine).  classes: packed_class_array; weights: packed scalars by global (class-major) index
    (1 per proof under Protocol 2, 3 under Protocol 1) or None with a 32-byte seed.  records: the classes' blocks in descending k
    (stable), class c's at rec_byte_off[c]; extra pairs: the classes' blocks in the given order."""
    lib = _native.load()
    arr, keep, total, rec_bytes, pairs = packed_class_array(protocol, classes)
    rec, pts, sc, status = (ctypes.create_string_buffer(max(nb, 1)) for nb in (rec_bytes, 64 * pairs, 32 * pairs, total))
    offs = (ctypes.c_uint64 * max(len(classes), 1))()
    vp = lambda b: ctypes.cast(b, ctypes.c_void_p)
    rc = lib.bpmi_ipa_batch_prepare_mixed(K, protocol, len(classes), ctypes.addressof(arr), weights, seed, threads, vp(rec), ctypes.addressof(offs), vp(pts), vp(sc),
                                          vp(status))
    del keep
    if rc != 0:
        raise EngineError("libbpmi error %d: %s" % (rc, lib.bpmi_last_error(None).decode()))
    return rec.raw[:rec_bytes], list(offs)[:len(classes)], pts.raw[: 64 * pairs], sc.raw[: 32 * pairs], status.raw[:total]


_default = None
_default_lock = threading.Lock()


def default_engine():
    """Process-wide engine (like the reference's PipSECP256k1 singleton it is stateless
    between calls).  Raises if libbpmi.so or the GPU is missing."""
    global _default
    with _default_lock:
        if _default is None:
            _default = Engine()
        return _default


def set_default_engine(engine):
    global _default
    with _default_lock:
        _default = engine
