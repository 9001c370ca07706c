"""Every option of bpmi_set_option: its default, the accepted values at the edges of what it takes, the nearest refused values, the
message of a refused value, and what a successful set does beyond storing the value.  Transcribed from the strcmp chain bpmi_set_option
was before the table of python-bulletproofs_amd/csrc/options_host.hpp replaced it; tests/test_options_cpu.py holds the table against
this list, tests/test_gpu_abi_errors.py the entry point itself.

effect: "none" | "graphs" (the captured launch sequences are dropped) | "graphs_if_zero" (only when the value is 0) | "fold_keys" (the
ctx forgets whose fold tables it holds)."""
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)


def _flag(name, default, effect="none"):
    return (name, default, [0, 1], [-1, 2, I64_MIN, I64_MAX], "%s must be 0 or 1" % name, effect)


# (name, default, accepted, refused, message, effect)
CASES = [
    ("window_bits", 0, [0, 2, 3, 16], [-1, 1, 17, I64_MIN, I64_MAX], "window_bits must be 0 or 2..16", "none"),
    ("accum_stream", 0, [0, 1, 2], [-1, 3], "accum_stream must be 0, 1 or 2", "none"),
    ("lane_priority", 0, [-1, 0, 1], [-2, 2], "lane_priority must be -1, 0 or 1", "none"),
    _flag("h2c_plain", 0),
    ("msm_batch_route", 0, [0, 3], [-1, 4], "msm_batch_route must be 0 .. 3", "none"),
    ("msm_batch_vecs", 0, [0, 1 << 20], [-1, (1 << 20) + 1], "msm_batch_vecs must be 0 .. 2^20", "none"),
    ("h2c_per_lane", 0, [0, 1, 64], [-1, 65], "h2c_per_lane must be 0 .. 64", "none"),
    _flag("pair_sched", 0),
    ("prover_wire_format", 2, [2, 3], [1, 4, 0, -2], "prover_wire_format must be 2 or 3", "none"),
    ("prover_split", 0, [0, 1, 1 << 20], [-1, (1 << 20) + 1], "prover_split must be 0, 1 or the smallest half", "none"),
    ("accum_runs", 1, [0, 1, 2], [-1, 3], "accum_runs must be 0, 1 or 2", "graphs"),
    ("accum_runs_cap", 0, [0, 1 << 30], [-1, (1 << 30) + 1], "accum_runs_cap must be 0 .. 2^30", "graphs"),
    ("rounds", 0, [0, 16], [-1, 17], "rounds must be 0 .. 16", "graphs"),
    _flag("pair_rounds", 0),
    _flag("accum_chain", 1),
    ("slice_n", 0, [-1, 0, 1 << 16, 1 << 23], [-2, 1, (1 << 16) - 1, (1 << 23) + 1], "slice_n must be -1, 0 or 2^16 .. 2^23", "none"),
    ("slice_min", 0, [0, 1 << 23], [-1, (1 << 23) + 1], "slice_min must be 0 .. 2^23", "none"),
    ("mid_parts", 0, [0, 4], [-1, 5], "mid_parts must be 0 .. 4", "graphs"),
    _flag("mixed_windows", 1, "graphs"),
    _flag("top_window_unsigned", 1, "graphs"),
    ("prover_job_lanes", 0, [0, 16, 64], [-1, 1, 15, 17, 32, 63, 65], "prover_job_lanes must be 0, 16 or 64", "none"),
    ("prover_table_bits", 0, [0, 4, 16], [-1, 1, 3, 17], "prover_table_bits must be 0 or 4..16", "none"),
    _flag("ipa_fixed_generators", 0, "fold_keys"),
    ("validate_points", 1, [0, 1, 2], [-1, 3], "validate_points must be 0, 1 or 2", "none"),
    _flag("hist_scan_fused", 0, "graphs"),
    _flag("reduce_fit", 1, "graphs"),
    ("final_spread", 3, [0, 3], [-1, 4], "final_spread must be 0 .. 3", "graphs"),
    _flag("sort_inblock", 1, "graphs"),
    _flag("segscan_fused", 0, "graphs"),
    ("priority", 1, [0, 1, 16, 31], [-1, 2, 15, 32], "priority must be 0, 1 or 16 + a mask of stages", "graphs"),
    ("hist_threads", 0, [0, 256, 512, 1024], [-1, 1, 255, 257, 128, 768, 1023, 1025, 2048], "hist_threads must be 0, 256, 512 or 1024", "none"),
    ("hist_blocks", 0, [0, 8192], [-1, 8193], "hist_blocks must be in [0, 8192]", "none"),
    _flag("direct_result", 1, "graphs"),
    _flag("graphs", 0, "graphs_if_zero"),
    _flag("tail_thread", 1),
    _flag("pair_chain", 0),
    ("mid_min", 0, [-1, 0, 8448], [-2, 8449], "mid_min must be -1 .. 8448", "graphs"),
    ("mid_single_min", 0, [-1, 0, 8448], [-2, 8449], "mid_single_min must be -1 .. 8448", "graphs"),
    _flag("small_pair", 1),
    _flag("fused_scan", 1),
    _flag("quad_final", 1),
    ("spin_wait", 0, [0, 10 ** 7], [-1, 10 ** 7 + 1], "spin_wait must be in [0, 10^7]", "none"),
    _flag("mul_batch_glv", 1),
    ("tail", 0, [0, 1, 2], [-1, 3], "tail must be 0, 1 or 2", "none"),
    ("small_n", 0, [-1, 0, 1 << 16], [-2, (1 << 16) + 1], "small_n must be -1 .. 65536", "none"),
    _flag("split", 0),
    _flag("async_lanes", 0),
    ("rp_only_role", -1, [-1, 0, 3], [-2, 4], "rp_only_role must be in [-1, 3]", "none"),
    ("glv", 0, [-1, 0, 1], [-2, 2], "glv must be -1, 0 or 1", "none"),
    ("rp_priority", 1, [0, 1, 2], [-1, 3], "rp_priority must be 0, 1 or 2", "none"),
    ("rp_slices", 0, [0, 4], [-1, 5], "rp_slices must be 0 .. 4", "none"),
    _flag("rp_overlap", 1),
    # (any non-negative 64-bit value is taken and narrowed to int as it is stored: a defect the table keeps, see its row)
    ("rp_rows", 0, [0, 1, (1 << 31) - 1, 1 << 31, I64_MAX], [-1, I64_MIN], "rp_rows must be >= 0", "none"),
    ("rp_lanes", 0, [0, 1, 2, 32, 64], [-1, 3, 63, 65, 128, I64_MIN], "rp_lanes must be 0 or a power of two <= 64", "none"),
    _flag("pair_phases", 0),
    ("fold_wnaf", 2, [0, 1, 2], [-1, 3], "fold_wnaf must be 0, 1 or 2", "none"),
    ("reduce_epl", 0, [0, 64], [-1, 65], "reduce_epl must be 0..64", "none"),
    ("chunk", 0, [0, 4096], [-1, 4097], "chunk must be 0..4096", "none"),
    _flag("ipa_small_step", 0),
    _flag("fold_shared", 1),
    ("ipa_small_m", 0, [0, 1, 2, 4096, 1 << 40, 1 << 62], [-1, 3, (1 << 40) + 1, I64_MAX, I64_MIN],
     "ipa_small_m must be 0 (default), 1 (never) or a power of two", "none"),
    ("ipa_big_m", 0, [0, 1, 2, 1 << 18, 1 << 40, 1 << 62], [-1, 3, (1 << 40) + 1, I64_MAX, I64_MIN], "ipa_big_m must be 0 or a power of two", "none"),
]
UNKNOWN = ["", "no_such_option", "window_bits ", "Window_bits", "opt_c"]


def probes():
    """(name, value, accepted, message or None, effect or None) for every value of every case, the default among the accepted ones."""
    out = []
    for name, default, good, bad, msg, effect in CASES:
        for v in dict.fromkeys([default] + good):
            out.append((name, v, True, None, effect))
        for v in bad:
            out.append((name, v, False, msg, None))
    return out
