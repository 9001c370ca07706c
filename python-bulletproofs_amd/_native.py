"""ctypes loader for libbpmi.so (include/bpmi.h).  There is no CPU fallback: if the
library or a gfx950 device is missing, everything that needs it raises."""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BPMI_LIB") or os.path.join(HERE, "libbpmi.so")      # BPMI_LIB: A/B experiments with two builds in one run
NSTAGES = 15

# name -> (restype, argtypes); this table is checked against include/bpmi.h by tests
_vp, _cp, _u64, _i, _sz = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_size_t
SIGNATURES = {
    "bpmi_version": (_i, []),
    "bpmi_device_count": (_i, []),
    "bpmi_ctx_create": (_vp, [_i, _vp]),
    "bpmi_ctx_destroy": (None, [_vp]),
    "bpmi_last_error": (_cp, [_vp]),
    "bpmi_sync": (_i, [_vp]),
    "bpmi_set_option": (_i, [_vp, _cp, ctypes.c_int64]),
    "bpmi_malloc": (_i, [_vp, _sz, ctypes.POINTER(_vp)]),
    "bpmi_free": (_i, [_vp, _vp]),
    "bpmi_upload": (_i, [_vp, _vp, _cp, _sz]),
    "bpmi_download": (_i, [_vp, _vp, _vp, _sz]),
    "bpmi_msm": (_i, [_vp, _cp, _cp, _u64, _cp]),
    "bpmi_msm2": (_i, [_vp, _cp, _cp, _u64, _cp, _cp, _cp, _u64, _cp]),
    "bpmi_msm_dev": (_i, [_vp, _vp, _vp, _u64, _cp]),
    "bpmi_msm_dev_enqueue": (_i, [_vp, _i, _vp, _vp, _u64]),
    "bpmi_msm_finish": (_i, [_vp, _i, _cp]),
    "bpmi_msm_geometry": (_i, [_vp, _u64, _i, ctypes.POINTER(ctypes.c_uint32)]),
    "bpmi_debug_msm_runs": (_i, [_vp, _i, ctypes.POINTER(ctypes.c_uint32)]),
    "bpmi_ec_mul_batch": (_i, [_vp, _cp, _cp, _u64, _cp]),
    "bpmi_ec_mul_batch_dev": (_i, [_vp, _vp, _vp, _u64, _vp]),
    "bpmi_ec_lincomb2_batch": (_i, [_vp, _cp, _cp, _cp, _cp, _u64, _cp]),
    "bpmi_ec_lincomb2_batch_dev": (_i, [_vp, _vp, _vp, _cp, _cp, _u64, _vp]),
    "bpmi_ec_sum": (_i, [_vp, _cp, _u64, _cp]),
    "bpmi_ec_sum_dev": (_i, [_vp, _vp, _u64, _cp]),
    "bpmi_ec_sum_dev_enqueue": (_i, [_vp, _vp, _u64, _vp]),
    "bpmi_ec_decompress_batch": (_i, [_vp, _cp, _u64, _cp, _cp]),
    "bpmi_ec_decompress_batch_dev": (_i, [_vp, _vp, _u64, _vp, _vp]),
    "bpmi_ec_hash_batch": (_i, [_vp, _cp, _vp, _u64, ctypes.c_uint32, _cp, _cp]),
    "bpmi_ec_hash_batch_dev": (_i, [_vp, _cp, _vp, _u64, ctypes.c_uint32, _vp, _cp]),
    "bpmi_ec_hash_range": (_i, [_vp, _cp, _u64, _u64, _u64, ctypes.c_uint32, _cp, _cp]),
    "bpmi_ec_hash_range_dev": (_i, [_vp, _cp, _u64, _u64, _u64, ctypes.c_uint32, _vp, _cp]),
    "bpmi_memcpy_dev": (_i, [_vp, _vp, _vp, _sz]),
    "bpmi_msm_segs_dev": (_i, [_vp, ctypes.c_uint32, _vp, _vp, _vp, _cp]),
    "bpmi_msm_batch": (_i, [_vp, _cp, _u64, _cp, _u64, _vp]),
    "bpmi_msm_batch_dev": (_i, [_vp, ctypes.c_uint32, _vp, _vp, _vp, _u64, _vp]),
    "bpmi_msm_batch_dev_enqueue": (_i, [_vp, ctypes.c_uint32, _vp, _vp, _vp, _u64, _vp]),
    "bpmi_fixed_base_create": (_i, [_vp, _cp, _u64, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_vp)]),
    "bpmi_fixed_base_create_dev": (_i, [_vp, _vp, _u64, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_vp)]),
    "bpmi_fixed_base_destroy": (None, [_vp]),
    "bpmi_fixed_base_info": (_i, [_vp, ctypes.POINTER(_u64)]),
    "bpmi_fixed_base_table": (_i, [_vp, ctypes.c_uint32, _u64, _u64, _cp]),
    "bpmi_msm_fixed": (_i, [_vp, _cp, _u64, _cp]),
    "bpmi_msm_fixed_dev": (_i, [_vp, _vp, _u64, _cp]),
    "bpmi_msm_fixed_dev_enqueue": (_i, [_vp, _i, _vp, _u64]),
    "bpmi_sc_dot": (_i, [_vp, _cp, _cp, _u64, _cp]),
    "bpmi_sc_dot_dev": (_i, [_vp, _vp, _vp, _u64, _cp]),
    "bpmi_sc_fold": (_i, [_vp, _cp, _cp, _cp, _cp, _u64, _cp]),
    "bpmi_sc_fold_dev": (_i, [_vp, _vp, _vp, _cp, _cp, _u64, _vp]),
    "bpmi_sc_svector": (_i, [_vp, _cp, _cp, ctypes.c_uint32, _cp, _cp, _cp, _cp, _cp]),
    "bpmi_ipa_verify_dev": (_i, [_vp, _vp, _vp, _vp, _u64, _cp, _cp, ctypes.c_uint32, _cp, _cp, _cp, _cp, _u64, _cp]),
    "bpmi_sc_svector_sum": (_i, [_vp, ctypes.c_uint32, _u64, _cp, _cp, _cp, _cp, _cp, _cp, _cp, _cp]),
    "bpmi_ipa_verify_batch_dev": (_i, [_vp, _vp, _vp, _vp, _u64, _u64, _cp, _cp, ctypes.c_uint32, _cp, _cp, _cp, _cp, _cp, _u64, _cp]),
    "bpmi_sc_svector_sum_mixed": (_i, [_vp, _u64, _u64, ctypes.POINTER(ctypes.c_uint32), _cp, _cp, _cp, _cp, _cp, _cp, _cp, _cp, ctypes.POINTER(_u64)]),
    "bpmi_ipa_verify_batch_mixed_dev": (_i, [_vp, _vp, _vp, _vp, _u64, _u64, ctypes.POINTER(ctypes.c_uint32), _cp, _cp, _cp, _cp, _cp, _cp, _cp, _u64, _cp]),
    "bpmi_ipa_create": (_i, [_vp, _cp, _cp, _cp, _cp, _u64, _cp, ctypes.POINTER(_vp)]),
    "bpmi_ipa_create_scaled": (_i, [_vp, _cp, _cp, _cp, _cp, _u64, _cp, _cp, ctypes.POINTER(_vp)]),
    "bpmi_ipa_create_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _cp, ctypes.POINTER(_vp)]),
    "bpmi_ipa_len": (_u64, [_vp]),
    "bpmi_ipa_round_LR": (_i, [_vp, _cp, _cp]),
    "bpmi_ipa_fold": (_i, [_vp, _cp, _cp]),
    "bpmi_ipa_finish": (_i, [_vp, _cp, _cp]),
    "bpmi_ipa_export": (_i, [_vp, _cp, _cp, _cp, _cp]),
    "bpmi_rp_batch_prepare": (_i, [ctypes.c_uint32, ctypes.c_uint32, _u64, _vp, _u64, ctypes.c_void_p, _cp, _cp, _i, _cp, _cp, _cp, _cp, ctypes.c_void_p]),
    "bpmi_mod_hash_range": (_i, [_cp, _u64, _u64, _u64, _i, _cp]),
    "bpmi_rp_poly_coeffs": (_i, [ctypes.c_uint32, ctypes.c_uint32, _i, _cp, _cp, _cp, _cp, _cp, _i, _cp, _cp]),
    "bpmi_rp_final_vectors": (_i, [ctypes.c_uint32, ctypes.c_uint32, _i, _cp, _cp, _cp, _cp, _cp, _cp, _i, _cp, _cp, _cp, _cp, _cp]),
    "bpmi_rp_verifier_vectors": (_i, [ctypes.c_uint32, ctypes.c_uint32, _i, _cp, _cp, _i, _cp, _cp, _cp]),
    "bpmi_rp_wire_v2_to_v1": (_i, [_vp, _u64, _vp, _u64, _vp, _u64, _vp, _vp]),
    "bpmi_rp_batch_prepare_dev": (_i, [_vp, ctypes.c_uint32, ctypes.c_uint32, _u64, _vp, _u64, _vp, _cp, _cp, _vp, _vp, _vp, _cp, _vp]),
    "bpmi_rp_batch_verify_dev": (_i, [_vp, ctypes.c_uint32, ctypes.c_uint32, _u64, _vp, _u64, _vp, _cp, _cp, _vp, _vp, _vp, _vp, _cp, _vp]),      # (v_points: bytes or a page-locked address)
    "bpmi_rp_batch_group_values_dev": (_i, [_vp, ctypes.c_uint32, ctypes.c_uint32, _u64, _vp, _u64, _vp, _cp, _cp, _vp, _vp, _vp, _vp, _u64, _vp, _vp]),
    "bpmi_rp_batch_verify_mixed_dev": (_i, [_vp, ctypes.c_uint32, _vp, ctypes.c_uint32, _cp, _cp, _vp, _vp, _vp, _cp, _vp]),      # (classes: an array of RpClass)
    # ctx, n_classes, classes, n_gens_max, group (n_classes x uint64), weights, seed, d_gens, d_points, d_scalars, values, value_off, status
    "bpmi_rp_batch_group_values_mixed_dev": (_i, [_vp, ctypes.c_uint32, _vp, ctypes.c_uint32, _vp, _cp, _cp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "bpmi_rp_prover_create": (_i, [_vp, ctypes.c_uint32, _cp, _cp, _cp, _cp, _cp, ctypes.POINTER(_vp)]),
    "bpmi_rp_prover_create_aggregated": (_i, [_vp, ctypes.c_uint32, ctypes.c_uint32, _cp, _cp, _cp, _cp, _cp, ctypes.POINTER(_vp)]),
    "bpmi_rp_prover_destroy": (None, [_vp]),
    "bpmi_rp_prove_batch_proof_bytes": (_u64, [_vp, _u64]),
    "bpmi_rp_prove_batch": (_i, [_vp, _u64, _cp, _cp, _cp, _vp, _vp, _u64, _vp]),
    "bpmi_rp_prover_commit_batch": (_i, [_vp, _u64, _cp, _cp, _vp]),
    "bpmi_rp_prover_last_ms": (_i, [_vp, ctypes.POINTER(ctypes.c_double)]),
    "bpmi_rp_prove_batch_proof_bytes_class": (_u64, [_vp, ctypes.c_uint32, _u64]),
    # pv, n_classes, classes (RpProveClass array), out, cap, out_off
    "bpmi_rp_prove_batch_mixed": (_i, [_vp, ctypes.c_uint32, _vp, _vp, _u64, _vp]),
    "bpmi_ipa_batch_prover_create": (_i, [_vp, ctypes.c_uint32, _cp, _cp, _cp, _cp, ctypes.POINTER(_vp)]),
    "bpmi_ipa_batch_prover_destroy": (None, [_vp]),
    "bpmi_ipa_prove_batch_transcript_bytes": (_u64, [_vp, _i, _u64]),
    "bpmi_ipa_prove_batch": (_i, [_vp, _i, _u64, _cp, _cp, _cp, _cp, _cp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "bpmi_ipa_batch_prover_last_ms": (_i, [_vp, ctypes.POINTER(ctypes.c_double)]),
    "bpmi_ipa_batch_prover_commit_batch": (_i, [_vp, _u64, _cp, _cp, _i, _cp, _vp]),
    "bpmi_ipa_batch_prover_commit_last_ms": (_i, [_vp, ctypes.POINTER(ctypes.c_double)]),
    "bpmi_ipa_prove_batch_transcript_bytes_class": (_u64, [_vp, ctypes.c_uint32, _i, _u64]),
    # pv, protocol | u_mode, n_classes, classes (IpaProveClass / IpaCommitClass array)
    "bpmi_ipa_prove_batch_mixed": (_i, [_vp, _i, ctypes.c_uint32, _vp]),
    "bpmi_ipa_batch_prover_commit_batch_mixed": (_i, [_vp, _i, ctypes.c_uint32, _vp]),
    # (k | ctx, k | ctx, g, h, hscale, n), protocol, n_proofs, ab, xs, LR, transcripts, tr_off, start, u, P, c, head, weights, seed, ...
    "bpmi_ipa_batch_prepare": (_i, [ctypes.c_uint32, _i, _u64, _cp, _cp, _cp, _cp, _vp, _vp, _cp, _cp, _cp, _cp, _cp, _cp, _i, _vp, _vp, _vp, _vp]),
    "bpmi_ipa_batch_prepare_dev": (_i, [_vp, ctypes.c_uint32, _i, _u64, _cp, _cp, _cp, _cp, _vp, _vp, _cp, _cp, _cp, _cp, _cp, _cp, _vp, _vp, _vp, _vp]),
    "bpmi_ipa_verify_batch_packed_dev": (_i, [_vp, _vp, _vp, _vp, _u64, _i, _u64, _cp, _cp, _cp, _cp, _vp, _vp, _cp, _cp, _cp, _cp, _cp, _cp, _vp, _vp]),
    "bpmi_ipa_group_values_packed_dev": (_i, [_vp, _vp, _vp, _vp, _u64, _i, _u64, _cp, _cp, _cp, _cp, _vp, _vp, _cp, _cp, _cp, _cp, _cp, _cp, _u64, _vp, _vp]),
    # (K | ctx, K | ctx, g, h, hscale, n_gens), protocol, n_classes, classes (an array of IpaPackedClass), weights, seed, ...
    "bpmi_ipa_batch_prepare_mixed": (_i, [ctypes.c_uint32, _i, ctypes.c_uint32, _vp, _cp, _cp, _i, _vp, _vp, _vp, _vp, _vp]),
    "bpmi_ipa_batch_prepare_mixed_dev": (_i, [_vp, ctypes.c_uint32, _i, ctypes.c_uint32, _vp, _cp, _cp, _vp, _vp, _vp, _vp, _vp]),
    "bpmi_ipa_verify_batch_packed_mixed_dev": (_i, [_vp, _vp, _vp, _vp, _u64, _i, ctypes.c_uint32, _vp, _cp, _cp, _vp, _vp]),
    # ... classes, group (n_classes x uint64), weights, seed, values, value_off (n_classes + 1 x uint64), status
    "bpmi_ipa_group_values_packed_mixed_dev": (_i, [_vp, _vp, _vp, _vp, _u64, _i, ctypes.c_uint32, _vp, _vp, _cp, _cp, _vp, _vp, _vp]),
    # BPIP2: (k, prefix_len); k, protocol, n_proofs, ab, xs, LR, transcripts, tr_off, start, blobs, cap, off, status; k, protocol, n_proofs, blobs, off,
    # ab, xs, LR, transcripts, cap, tr_off, start, status (the _dev form behind ctx); ctx, g, h, hscale, n, protocol, n_proofs, blobs, off, u, P, ...
    "bpmi_ipa_wire_bytes": (_u64, [ctypes.c_uint32, _u64]),
    "bpmi_ipa_wire_encode": (_i, [ctypes.c_uint32, _i, _u64, _cp, _cp, _cp, _cp, _vp, _vp, _vp, _u64, _vp, _vp]),
    "bpmi_ipa_wire_expand": (_i, [ctypes.c_uint32, _i, _u64, _cp, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "bpmi_ipa_wire_expand_dev": (_i, [_vp, ctypes.c_uint32, _i, _u64, _cp, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "bpmi_ipa_verify_batch_wire_dev": (_i, [_vp, _vp, _vp, _vp, _u64, _i, _u64, _cp, _vp, _cp, _cp, _cp, _cp, _vp, _vp]),
    "bpmi_debug_ipap_t_budget": (_i, [_vp, _u64]),
    "bpmi_host_alloc": (_i, [_vp, ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "bpmi_host_free": (_i, [_vp, _vp]),
    "bpmi_ipa_destroy": (None, [_vp]),
    "bpmi_ipa_prove_rounds": (_i, [_vp, _cp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, ctypes.c_uint32, _vp]),
    "bpmi_debug_fe_op": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _u64, _vp]),
    "bpmi_debug_quad_add": (_i, [_vp, _vp, _vp, _u64, _vp]),
    "bpmi_debug_point_op": (_i, [_vp, _i, _vp, _vp, _u64, _vp]),
    "bpmi_profile": (_i, [_vp, _i]),
    "bpmi_profile_reset": (_i, [_vp]),
    "bpmi_profile_read": (_i, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_u64)]),
    "bpmi_profile_stage_name": (_cp, [_i]),
}

_lib = None


class RpClass(ctypes.Structure):
    """bpmi_rp_class (include/bpmi.h): one class of bpmi_rp_batch_verify_mixed_dev.  The pointers are plain addresses: whoever fills the
    structure keeps the objects behind them alive for the call."""
    _fields_ = [("n_gens", ctypes.c_uint32), ("values_per_proof", ctypes.c_uint32), ("n_proofs", ctypes.c_uint64), ("blobs", ctypes.c_void_p),
                ("blobs_len", ctypes.c_uint64), ("blob_off", ctypes.c_void_p), ("v_points", ctypes.c_void_p)]


class RpProveClass(ctypes.Structure):
    """bpmi_rp_prove_class (include/bpmi.h): one class of bpmi_rp_prove_batch_mixed.  Plain addresses, as RpClass."""
    _fields_ = [("m", ctypes.c_uint32), ("n_proofs", ctypes.c_uint64), ("values", ctypes.c_void_p), ("gammas", ctypes.c_void_p), ("seeds", ctypes.c_void_p),
                ("seed_off", ctypes.c_void_p)]


class IpaProveClass(ctypes.Structure):
    """bpmi_ipa_prove_class (include/bpmi.h): one class of bpmi_ipa_prove_batch_mixed, its inputs and its own outputs.  Plain addresses, as RpClass."""
    _fields_ = ([("n", ctypes.c_uint32), ("n_proofs", ctypes.c_uint64)] +
                [(name, ctypes.c_void_p) for name in ("a", "b", "c", "P", "seeds", "seed_off", "ab", "xs", "LR", "head", "transcripts")] +
                [("cap", ctypes.c_uint64), ("tr_off", ctypes.c_void_p)])


class IpaCommitClass(ctypes.Structure):
    """bpmi_ipa_commit_class (include/bpmi.h): one class of bpmi_ipa_batch_prover_commit_batch_mixed.  Plain addresses, as RpClass."""
    _fields_ = [("n", ctypes.c_uint32), ("count", ctypes.c_uint64)] + [(name, ctypes.c_void_p) for name in ("a", "b", "t", "out")]


class IpaPackedClass(ctypes.Structure):
    """bpmi_ipa_packed_class (include/bpmi.h): one class of the mixed packed inner-product calls.  Plain addresses, as RpClass."""
    _fields_ = [("k", ctypes.c_uint32), ("n_proofs", ctypes.c_uint64)] + [(name, ctypes.c_void_p) for name in
                ("ab", "xs", "LR", "transcripts", "tr_off", "start", "u", "P", "c", "head")]


class NativeLibraryMissing(RuntimeError):
    pass


def load():
    """Load libbpmi.so and declare every entry point; raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryMissing(
            "libbpmi.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'`; "
            "there is no CPU fallback for the MSM / IPA path." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = header / library drift
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
