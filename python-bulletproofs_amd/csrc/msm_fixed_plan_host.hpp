// msm_fixed_plan_host.hpp -- part of libbpmi; plain C++17 (no HIP, no bpmi_ctx), also compiled for the host by tests/csrc_host.
// The plan of a fixed-base MSM (bpmi_fixed_base_*, bpmi_msm_fixed*) as pure functions: the argument errors, window bits c, the W uniform
// signed windows, the table rows R and the Wv = ceil(W / R) virtual windows, the automatic rule, the map of a real window onto a
// (virtual window, row) slot, the table's size and the virtual geometry the bucket pipeline runs.
//
// The object keeps T[r][i] = 2^(c Wv r) P_i for r < R.  Digit w of scalar i weighs 2^(c w) = 2^(c (w % Wv)) 2^(c Wv (w / Wv)): it is an
// entry for point T[w / Wv][i] in window w % Wv.  So the MSM of n pairs in W windows is the bucket pipeline over n R virtual pairs
// (virtual pair r n + i is T[r][i]) in Wv windows: as many bucket additions, and only Wv windows for the bucket reduction and the tail.
// R = 1 is the ordinary MSM; R = W has one bucket set and no doubling in the tail.
// tests/test_msm_fixed_plan_cpu.py checks all of it without a GPU; msm_fixed_host.hpp consumes it, k_fixed_recode uses the map.
#pragma once
#include "msm_plan_host.hpp"

#define FIXED_C_MIN 10u                      // the LDS sort's range (msm_lds_sort): narrower windows would need sort path 1
#define FIXED_C_MAX 16u
#define FIXED_PAIRS_MAX SLICE_N_LIMIT        // n R: the sorted entry's 23-bit pair index (k_fine_sort_part: e & 0x7FFFFF)

static inline u32 fixed_windows(u32 c) { return 255u / c + 1u; }                 // uniform signed windows, no mixed widths
static inline u32 fixed_virtual_windows(u32 W, u32 rows) { return (W + rows - 1u) / rows; }
static inline u32 fixed_effective_rows(u32 W, u32 Wv) { return (W + Wv - 1u) / Wv; }   // rows that hold a window at all
// real window w -> virtual window and table row.  The one definition: the recoding kernel calls it for every digit it writes
struct FixedSlot { u32 wv, r; };
BPMI_HD FixedSlot fixed_window_slot(u32 w, u32 Wv) { FixedSlot s; s.wv = w % Wv; s.r = w / Wv; return s; }

struct FixedPlan {
  int err = 0; const char *msg = nullptr;      // an argument error: nothing else is set
  uint64_t n = 0;                              // points
  u32 c = 0, W = 0;                            // window bits, real windows.  c = 0: R = 1 by the automatic rule -- the ordinary MSM under the ctx's own options
  u32 R = 0, Wv = 0;                           // effective table rows, virtual windows
  uint64_t table_bytes = 0;                    // 64 n R
};
static inline FixedPlan fixed_plan_error(const char *msg) { FixedPlan p; p.err = BPMI_E_ARG; p.msg = msg; return p; }

// The automatic rule (window_bits = 0 and rows = 0), from profiles/r14_msm_fixed.txt (tools/bench_msm_fixed.py on MI355X; medians of 24
// alternating calls, ms one at a time, table against bpmi_msm_dev; the baseline's medians over a process's 16 .. 20 configurations spread
// 1.0 .. 3.0 %): per measured size the (c, R) with the lowest median, where it beats the baseline by more than that spread, and the band
// of a size runs to the next measured one.
//   2^13: (16, 16) 0.173 against 0.190 (-8.8 %; spread 1.0 %)        2^14: (16, 8) 0.179 against 0.227 (-21 %; 2.0 %)
//   2^16: (16, 4)  0.229 against 0.268 (-15 %; 2.2 %)                2^18: (16, 4) 0.396 against 0.466 (-15 %; 2.5 %)
//   2^19, 2^20: no (c, R) wins -- the best table, (16, 2), is 0.630 against 0.625 and 1.164 against 1.011: from 2^19 pairs the ordinary MSM
//   accumulates by runs and a window group does not -- so R = 1 above 2^18; below 2^13 nothing is measured: R = 1.
// With a table, 13 .. 15 bits lose to 16 at every size measured.
struct FixedAuto { u32 c, rows; };
static inline FixedAuto fixed_auto_rule(uint64_t n) {
  if (n < (1u << 13) || n > (1u << 18)) return FixedAuto{0u, 1u};
  if (n < (1u << 14)) return FixedAuto{16u, 16u};
  if (n < (1u << 16)) return FixedAuto{16u, 8u};
  return FixedAuto{16u, 4u};
}

// window_bits: 0 or 10 .. 16; rows: 0 or 1 .. W.  Both 0: the automatic rule.  One of them 0: that one is chosen -- window bits 16, or the
// most rows the pair bound allows -- around the explicit other, which is never overridden.
static inline FixedPlan fixed_plan(uint64_t n, u32 window_bits, u32 rows) {
  if (n == 0) return fixed_plan_error("n must be at least 1");
  if (n > BPMI_MAX_N) return fixed_plan_error("n exceeds BPMI_MAX_N");
  if (window_bits != 0 && (window_bits < FIXED_C_MIN || window_bits > FIXED_C_MAX)) return fixed_plan_error("window_bits must be 0 or 10 .. 16");
  if (rows > fixed_windows(window_bits ? window_bits : FIXED_C_MIN)) return fixed_plan_error("rows must be 0 or 1 .. W = 255 / window_bits + 1");
  FixedPlan p;
  p.n = n;
  u32 c = window_bits, R = rows;
  if (!c && !R) {
    const FixedAuto a = fixed_auto_rule(n);
    c = a.c; R = a.rows;
    if (c) while (R > 1u && n * fixed_effective_rows(fixed_windows(c), fixed_virtual_windows(fixed_windows(c), R)) > FIXED_PAIRS_MAX) R--;      // (lowers R until the bound holds)
    if (R <= 1u) { c = 0; R = 1; }
  } else if (!c) {
    c = FIXED_C_MAX;
    if (R > fixed_windows(c)) return fixed_plan_error("rows must be 0 or 1 .. W = 255 / window_bits + 1");
  } else if (!R) {
    R = fixed_windows(c);
    while (R > 1u && n * fixed_effective_rows(fixed_windows(c), fixed_virtual_windows(fixed_windows(c), R)) > FIXED_PAIRS_MAX) R--;
  }
  if (c) {
    p.c = c; p.W = fixed_windows(c);
    p.Wv = fixed_virtual_windows(p.W, R);
    p.R = fixed_effective_rows(p.W, p.Wv);
  } else { p.R = 1; }
  if (n * p.R > FIXED_PAIRS_MAX) return fixed_plan_error("n x rows exceeds 2^23 (the sorted entry holds a 23-bit pair index)");
  p.table_bytes = 64ull * n * p.R;
  return p;
}

// The geometry of the recoding: n real scalars in W uniform windows of c bits (for_each_digit_raw reads n, c, W, w0, top2)
static inline MsmGeom fixed_real_geometry(const FixedPlan &p) {
  MsmGeom g;
  memset(&g, 0, sizeof(g));
  g.n = (u32)p.n; g.c = p.c; g.W = p.W; g.w0 = 0; g.top2 = 0; g.B = 1u << (p.c - 1u); g.G = g.W * g.B;
  return g;
}
// The virtual geometry (R > 1): what msm_pick_geometry gives a pipeline MSM of n R pairs with forced window bits and a window group of
// Wv windows -- uniform widths (top2 = 0), w0 = 0, and L, nv, prio, fuse, inblock and runs by that function's own rules ("accum_runs" = 2
// plans the accumulation by runs, as for every window group).  The workspace is msm_layout of this geometry.
static inline MsmPlan fixed_virtual_geometry(const BpmiOptions &o, const MsmMode &mode, const FixedPlan &p) {
  BpmiOptions v = o;
  v.opt_c = (int)p.c;
  return msm_pick_geometry(v, mode, p.n * p.R, 0, p.Wv);
}
