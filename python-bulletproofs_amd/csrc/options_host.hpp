// options_host.hpp -- part of libbpmi; plain C++17 (no HIP), also compiled for the host by tests/csrc_host.
// The options of bpmi_set_option (include/bpmi.h) as ONE table over BpmiOptions (shared_defs.hpp, which keeps the defaults and says
// what each option does): a row is the name, the member it sets, the values it accepts, the message of a refused value and what a
// successful set does to the ctx beyond the member.  option_set is the whole of bpmi_set_option but the ctx; the tests address
// options through option_find by the same names (tests/test_options_cpu.py pins every row).
#pragma once
#include <stdint.h>
#include <string.h>
#include <string>

#include "shared_defs.hpp"

enum OptionEffect {
  OPT_FX_NONE = 0,
  OPT_FX_GRAPHS,              // the captured launch sequences were planned under the old value: drop them (msm_graphs_clear)
  OPT_FX_GRAPHS_IF_ZERO,      // ... only when the option is switched off ("graphs")
  OPT_FX_FOLD_KEYS            // forget whose fold tables the ctx holds ("ipa_fixed_generators")
};
struct OptionRow {
  const char *name;
  int BpmiOptions::*i32;               // the member, one of the two
  int64_t BpmiOptions::*i64;
  int64_t lo, hi;                      // accepted: lo <= value <= hi, or, where that is no range, ...
  bool (*accepts)(int64_t);            // ... this
  const char *msg;
  OptionEffect fx;
  bool ok(int64_t v) const { return accepts ? accepts(v) : v >= lo && v <= hi; }
  int64_t get(const BpmiOptions &o) const { return i32 ? o.*i32 : o.*i64; }
  void put(BpmiOptions &o, int64_t v) const { if (i32) o.*i32 = (int)v; else o.*i64 = v; }
};
namespace option_rows {
typedef int BpmiOptions::*M32;
typedef int64_t BpmiOptions::*M64;
constexpr OptionRow range(const char *name, M32 m, int64_t lo, int64_t hi, const char *msg, OptionEffect fx = OPT_FX_NONE) { return {name, m, nullptr, lo, hi, nullptr, msg, fx}; }
constexpr OptionRow flag(const char *name, M32 m, const char *msg, OptionEffect fx = OPT_FX_NONE) { return range(name, m, 0, 1, msg, fx); }
constexpr OptionRow pred(const char *name, M32 m, bool (*f)(int64_t), const char *msg, OptionEffect fx = OPT_FX_NONE) { return {name, m, nullptr, 0, 0, f, msg, fx}; }
constexpr OptionRow pred(const char *name, M64 m, bool (*f)(int64_t), const char *msg) { return {name, nullptr, m, 0, 0, f, msg, OPT_FX_NONE}; }
inline bool zero_or_pow2(int64_t v) { return v >= 0 && !(v & (v - 1)); }
typedef BpmiOptions O;
static const OptionRow ROWS[] = {
  pred("window_bits", &O::opt_c, [](int64_t v) { return v == 0 || (v >= 2 && v <= 16); }, "window_bits must be 0 or 2..16"),
  range("accum_stream", &O::opt_accum_stream, 0, 2, "accum_stream must be 0, 1 or 2"),
  range("lane_priority", &O::opt_lane_prio, -1, 1, "lane_priority must be -1, 0 or 1"),
  flag("h2c_plain", &O::opt_h2c_plain, "h2c_plain must be 0 or 1"),
  range("msm_batch_route", &O::opt_msm_batch_route, 0, 3, "msm_batch_route must be 0 .. 3"),
  range("msm_batch_vecs", &O::opt_msm_batch_vecs, 0, 1 << 20, "msm_batch_vecs must be 0 .. 2^20"),
  range("h2c_per_lane", &O::opt_h2c_per_lane, 0, 64, "h2c_per_lane must be 0 .. 64"),
  flag("pair_sched", &O::opt_pair_sched, "pair_sched must be 0 or 1"),
  pred("prover_wire_format", &O::opt_prover_wire, [](int64_t v) { return v == 2 || v == 3; }, "prover_wire_format must be 2 or 3"),
  range("prover_split", &O::opt_prover_split, 0, 1 << 20, "prover_split must be 0, 1 or the smallest half"),
  range("accum_runs", &O::opt_accum_runs, 0, 2, "accum_runs must be 0, 1 or 2", OPT_FX_GRAPHS),
  range("accum_runs_cap", &O::opt_accum_runs_cap, 0, 1 << 30, "accum_runs_cap must be 0 .. 2^30", OPT_FX_GRAPHS),
  range("rounds", &O::opt_rounds, 0, 16, "rounds must be 0 .. 16", OPT_FX_GRAPHS),
  flag("pair_rounds", &O::opt_pair_rounds, "pair_rounds must be 0 or 1"),
  flag("accum_chain", &O::opt_accum_chain, "accum_chain must be 0 or 1"),
  pred("slice_n", &O::opt_slice_n, [](int64_t v) { return v == -1 || v == 0 || (v >= (1 << 16) && v <= (1 << 23)); }, "slice_n must be -1, 0 or 2^16 .. 2^23"),
  range("slice_min", &O::opt_slice_min, 0, 1 << 23, "slice_min must be 0 .. 2^23"),
  range("mid_parts", &O::opt_mid_parts, 0, 4, "mid_parts must be 0 .. 4", OPT_FX_GRAPHS),
  flag("mixed_windows", &O::opt_mixed, "mixed_windows must be 0 or 1", OPT_FX_GRAPHS),
  flag("top_window_unsigned", &O::opt_top2, "top_window_unsigned must be 0 or 1", OPT_FX_GRAPHS),
  pred("prover_job_lanes", &O::opt_prover_job_lanes, [](int64_t v) { return v == 0 || v == 16 || v == 64; }, "prover_job_lanes must be 0, 16 or 64"),
  pred("prover_table_bits", &O::opt_prover_tw, [](int64_t v) { return v == 0 || (v >= 4 && v <= 16); }, "prover_table_bits must be 0 or 4..16"),
  flag("ipa_fixed_generators", &O::opt_ipa_fixed, "ipa_fixed_generators must be 0 or 1", OPT_FX_FOLD_KEYS),
  range("validate_points", &O::opt_validate, 0, 2, "validate_points must be 0, 1 or 2"),
  flag("hist_scan_fused", &O::opt_histscan, "hist_scan_fused must be 0 or 1", OPT_FX_GRAPHS),
  flag("reduce_fit", &O::opt_reduce_fit, "reduce_fit must be 0 or 1", OPT_FX_GRAPHS),
  range("final_spread", &O::opt_final_spread, 0, 3, "final_spread must be 0 .. 3", OPT_FX_GRAPHS),
  flag("sort_inblock", &O::opt_inblock, "sort_inblock must be 0 or 1", OPT_FX_GRAPHS),
  flag("segscan_fused", &O::opt_segfuse, "segscan_fused must be 0 or 1", OPT_FX_GRAPHS),
  pred("priority", &O::opt_prio, [](int64_t v) { return v == 0 || v == 1 || (v >= 16 && v <= 31); }, "priority must be 0, 1 or 16 + a mask of stages", OPT_FX_GRAPHS),
  pred("hist_threads", &O::opt_hist_threads, [](int64_t v) { return v == 0 || v == 256 || v == 512 || v == 1024; }, "hist_threads must be 0, 256, 512 or 1024"),
  range("hist_blocks", &O::opt_hist_blocks, 0, 8192, "hist_blocks must be in [0, 8192]"),
  flag("direct_result", &O::opt_direct, "direct_result must be 0 or 1", OPT_FX_GRAPHS),
  flag("graphs", &O::opt_graph, "graphs must be 0 or 1", OPT_FX_GRAPHS_IF_ZERO),
  flag("tail_thread", &O::opt_tail_thread, "tail_thread must be 0 or 1"),
  flag("pair_chain", &O::opt_pair_chain, "pair_chain must be 0 or 1"),
  range("mid_min", &O::opt_mid_min, -1, MID_NMAX, "mid_min must be -1 .. 8448", OPT_FX_GRAPHS),
  range("mid_single_min", &O::opt_mid_single, -1, MID_NMAX, "mid_single_min must be -1 .. 8448", OPT_FX_GRAPHS),
  flag("small_pair", &O::opt_pair1, "small_pair must be 0 or 1"),
  flag("fused_scan", &O::opt_fuse, "fused_scan must be 0 or 1"),
  flag("quad_final", &O::opt_quad, "quad_final must be 0 or 1"),
  range("spin_wait", &O::opt_spin_wait, 0, 10000000, "spin_wait must be in [0, 10^7]"),
  flag("mul_batch_glv", &O::opt_mulb, "mul_batch_glv must be 0 or 1"),
  range("tail", &O::opt_tail, 0, 2, "tail must be 0, 1 or 2"),
  range("small_n", &O::opt_small, -1, 1 << 16, "small_n must be -1 .. 65536"),
  flag("split", &O::opt_split, "split must be 0 or 1"),
  flag("async_lanes", &O::opt_async_lanes, "async_lanes must be 0 or 1"),
  range("rp_only_role", &O::opt_rp_only_role, -1, 3, "rp_only_role must be in [-1, 3]"),
  range("glv", &O::opt_glv, -1, 1, "glv must be -1, 0 or 1"),
  range("rp_priority", &O::opt_rp_prio, 0, 2, "rp_priority must be 0, 1 or 2"),
  range("rp_slices", &O::opt_rp_slices, 0, 4, "rp_slices must be 0 .. 4"),
  flag("rp_overlap", &O::opt_rp_overlap, "rp_overlap must be 0 or 1"),
  range("rp_rows", &O::opt_rp_rows, 0, INT64_MAX, "rp_rows must be >= 0"),      // (any non-negative value, narrowed to int as it is stored)
  pred("rp_lanes", &O::opt_rp_lanes, [](int64_t v) { return v == 0 || (v >= 1 && v <= 64 && !(v & (v - 1))); }, "rp_lanes must be 0 or a power of two <= 64"),
  flag("pair_phases", &O::opt_pair_phases, "pair_phases must be 0 or 1"),
  range("fold_wnaf", &O::opt_fold_wnaf, 0, 2, "fold_wnaf must be 0, 1 or 2"),
  range("reduce_epl", &O::opt_epl, 0, 64, "reduce_epl must be 0..64"),
  range("chunk", &O::opt_chunk, 0, 4096, "chunk must be 0..4096"),
  flag("ipa_small_step", &O::opt_ipa_step, "ipa_small_step must be 0 or 1"),
  flag("fold_shared", &O::opt_fold_shared, "fold_shared must be 0 or 1"),
  pred("ipa_small_m", &O::opt_ipa_small, zero_or_pow2, "ipa_small_m must be 0 (default), 1 (never) or a power of two"),
  pred("ipa_big_m", &O::opt_ipa_big, zero_or_pow2, "ipa_big_m must be 0 or a power of two"),
};
}  // namespace option_rows
#define OPTION_NROWS ((int)(sizeof(option_rows::ROWS) / sizeof(option_rows::ROWS[0])))

// the row of a bpmi_set_option name, nullptr: no such option
static inline const OptionRow *option_find(const char *name) {
  for (const OptionRow &r : option_rows::ROWS) if (!strcmp(name, r.name)) return &r;
  return nullptr;
}
// BPMI_OK with the effect the caller owes the ctx, or BPMI_E_ARG with the message; `o` changes only on BPMI_OK
struct OptionSet { int rc; OptionEffect fx; std::string msg; };
static inline OptionSet option_set(BpmiOptions &o, const char *name, int64_t value) {
  const OptionRow *r = option_find(name);
  if (!r) return {BPMI_E_ARG, OPT_FX_NONE, std::string("unknown option ") + name};
  if (!r->ok(value)) return {BPMI_E_ARG, OPT_FX_NONE, r->msg};
  r->put(o, value);
  return {BPMI_OK, r->fx, std::string()};
}
