// msm_plan_host.hpp -- part of libbpmi; plain C++17 (no HIP, no bpmi_ctx), also compiled for the host by tests/csrc_host.
// The plan of one MSM as pure functions of (options, mode, sizes): kernel family, window bits, mixed-width windows, chunk length,
// workspace layout, the bucket reduction's jobs and tail offsets, slices.  Everything that decides a buffer size or a launch shape
// is here, where tests/test_msm_plan_cpu.py checks it without a GPU; msm_host.hpp queues what these functions return.
#pragma once
#include <algorithm>

#include "shared_defs.hpp"

struct MsmGeom {
  u32 n;       // pairs (with GLV: virtual pairs = 2 x the caller's)
  u32 c;       // window bits
  u32 W;       // windows handled by this launch sequence: [w0, w0 + W) of the recoding
  u32 w0;      // first window (> 0 when one MSM is split into window groups on two lanes)
  u32 B;       // buckets per window = 2^(c-1)
  u32 G;       // W * B
  u32 L;       // entries per thread in k_accum_l0
  u32 nv;      // partial sums per window that the bucket reduction hands to the tail (1 or 4)
  u32 prio;    // mask of the stages (PRIO_*) whose kernels raise their waves' issue priority (see raise_priority)
  u32 fuse;    // 1: k_accum_l0 folds the partial records of a wave's 64 chunks itself (two records per WAVE go to k_segscan, not two per thread)
  u32 top2;    // Wb, the number of WIDE windows (round 5): the last Wb of the W windows have c + 1 bits and 2B buckets each, chosen so that
               // (W - Wb) c + Wb (c + 1) = 256 -- the windows cover exactly the 256 bit positions, the top bit of a folded scalar (< 2^255)
               // is 0, so the last window's digit never exceeds its 2^c and there is NO carry window and no short one (a window of a few
               // bits is one partition of n entries for the sort and a handful of giant buckets for the accumulation).  c = 15: 16 + 1
               // windows; c = 13: 10 + 9; c = 12: 17 + 4.  Keys of window w start at (w + max(0, w - (W - Wb))) B;  G = (W + Wb) B.  0: uniform
  u32 runs;    // 1: the accumulation by runs is planned -- k_accum_runs adds one whole bucket per thread, buckets in order of their length, unless the
               // device finds a run longer than the cap (msm_runs_cap); then k_accum_l0 and k_segscan, queued behind it every time, do the work
  u32 inblock; // 1 (n <= 2^17): k_fine_sort_part sorts a partition of ANY size itself (a heavy one without the LDS staging buffer);
               // the two tile kernels for heavy partitions are not launched
};
// one job of k_digit_sums / the finish kernels (the bucket reduction by two-position digit sums, msm_kernels.hpp)
struct DigitJob {
  u32 in_off, in_stride;     // array a starts at record a * in_stride + in_off of X
  u32 N, s, type;            // entries, split bits, 0 = D0 (by lo) / 1 = D1 (by hi)
  u32 glanes, gpw;           // lanes per sum (1 .. 64, any value) and sums per wave = 64 / glanes: a sum never straddles two waves
  u32 nsums;                 // sums per array: 2^s - 1 (type 0) or N >> s (type 1)
  u32 out_off, out_stride;   // sum idx (1-based) of array a -> record a * out_stride + out_off + idx - 1 of D
  u32 blk0;                  // first block of this job
  u32 cnt;                   // arrays (windows) of this job
};
struct DigitJobs { DigitJob j[4]; u32 njobs, prio; };

// What the caller's pipeline does around this MSM (an argument of the plan and of msm_enqueue, never state of the ctx):
struct MsmMode {
  bool chained = false;    // its accumulation is ordered behind the one queued before it on another lane (bpmi_msm_dev_enqueue with
                           // async_lanes, the slices of a large MSM, a pair under pair_chain / pair_sched)
  bool free_run = false;   // ... chained, but NOT ordered (option accum_chain = 0: the lanes run free)
  bool beside = false;     // a synchronous pair of large MSMs: another MSM's kernels run beside this accumulation (msm_run_pair)
};
struct MsmPlan { MsmGeom g; bool mid, small, glv; };
// sort path 2 (the two-level LDS partition sort) takes a bucket-pipeline MSM when the bucket key has more than 8 bits and the packed entry
// (8-bit lo | sign | 23-bit index) fits; path 1 (global atomics) otherwise.  The one place that says so: msm_layout's w.P and MsmGeom.runs read it.
static inline bool msm_lds_sort(u32 c, u32 n) { return c >= 10u && n <= (1u << 23); }      // mid: the one-block-per-window kernel, small: the one-launch kernel, neither: the bucket pipeline

// Window bits from the tools/tune_msm.py sweeps on MI355X (profiles/r01_tune_msm_after_sort_and_reduce_rewrites.txt).
// Besides the usual bucket-count trade-off, windows whose TOP window holds only a few
// bits (255 mod c small: c = 15, 14, 12, 11) concentrate a whole window's digits in a
// handful of buckets, so c in {8, 16} (top window 7, 15 bits) are preferred.
// the 12-bit mixed-width pipeline's lower end (when the one-block-per-window kernel is switched off; with it -- three blocks per window --
// that kernel keeps its whole range for single MSMs too: 8 192 pairs 0.184 ms against 0.207, profiles/r05_mid_kernel_parts_ab.txt)
#define MID_SINGLE_MAX_MIXED 5632u
static inline u32 pick_window_bits(const BpmiOptions &o, uint64_t n) {
  if (o.opt_c >= 2 && o.opt_c <= 16) return (u32)o.opt_c;
  // Round 5, with mixed window widths (MsmGeom.top2: no carry window and no short top window at ANY width; tools/r05_exp_mixed.sh,
  // profiles/r05_mixed_window_widths_sweep.txt): 12 bits (17 + 4 windows, 51 k buckets) from the end of the one-block kernel's range (8 448)
  // to 19 000 pairs, 13 bits (10 + 9 windows, 115 k buckets) to 185 000 -- 2^16: 0.272 ms against 0.299 for c = 15 and 0.311 for c = 16 --,
  // 16 bits beyond (14 / 15 tie with it around 2 x 10^5 and lose above).  Without them: the table of the first half of the round
  // (c = 15 with its one wide window from 15 360 to 2^17, 12 from 10 240, 8 below; profiles/r05_window_table_sweep.txt)
  if (o.opt_mixed && o.opt_top2) {
    if (n >= 185000u) return 16;
    if (n >= 19000u) return 13;
    if (n >= MID_SINGLE_MAX_MIXED) return 12;
  } else {
    if (n >= (1u << 17)) return 16;
    if (n >= 15360u) return o.opt_top2 ? 15 : 16;
    if (n >= 10240u) return 12;
  }
  if (n >= (1u << 10)) return 8;
  u32 lg = 0;
  while ((1ull << (lg + 1)) <= n) lg++;
  const int c = (int)lg - 2;
  return (u32)(c < 4 ? 4 : c);
}

// tools/try_small.py (profiles/r04_small_msm_vs_bucket_pipeline.txt): the one-launch kernel wins up to 2^12 pairs (0.21 ms against
// 0.26) and loses at 2^13 (0.33 against 0.29); the threshold sits just above 4 097 = the L / R of an inner-product round over
// 4 096 generators (a 64-bit x 32 aggregated range proof; every late round of a larger proof after its product fold)
#define SMALL_N_DEFAULT 4608
// a PAIR of MSMs (bpmi_msm2, the L / R of an inner-product round) whose larger one has this many pairs or more, up to MID_NMAX, is ONE
// launch of k_msm_mid (option "mid_min": 0 default, -1 never)
#define MID_MIN_DEFAULT 1536
#define MID_SINGLE_MIN_DEFAULT 2560      // one MSM at a time (option "mid_single_min": 0 default, -1 never)

// blocks per window of k_msm_mid (option "mid_parts": 0 = this rule, 1 .. 4 forced): from 3 000 pairs three -- a part more costs every window
// one more addition in the host tail (~13 us per result), a third of the pairs less per block saves 18 us at 2 049 pairs, 37 at 4 097, 70 at 8 193
static inline u32 mid_parts(const BpmiOptions &o, uint64_t n) {
  if (o.opt_mid_parts >= 1 && o.opt_mid_parts <= 4) return (u32)o.opt_mid_parts;
  return n >= 3000u ? 3u : 1u;
}

// The geometry of one MSM of n pairs: which kernel family, window bits, windows, buckets, chunk length.  A function of its arguments
// only -- the options, the mode, n and the window group [w0, w0 + wcount) (wcount = 0: all windows): msm_enqueue computes it,
// bpmi_msm_geometry reports it (bench.py's multiply-add count).  The mode moves the chunk length g.L alone, and only from 2^19 pairs.
static inline MsmPlan msm_pick_geometry(const BpmiOptions &o, const MsmMode &mode, uint64_t n, u32 w0, u32 wcount) {
  MsmPlan pl{};
  MsmGeom &g = pl.g;
  g.n = (u32)n;
  const uint64_t small_max = o.opt_small < 0 ? 0 : (o.opt_small ? (uint64_t)o.opt_small : SMALL_N_DEFAULT);
  // the one-block-per-window bucket kernel (k_msm_mid) between the small-MSM kernel and the pipeline
  // (measured, profiles/r04_mid_kernel_latency.txt: one MSM at a time it wins from ~2 500 pairs -- 0.18 ms against 0.21 at 3 000, 0.25
  // against 0.29 at 8 193 --, a PAIR in one launch from ~1 500 pairs each: 0.29 ms against 0.44 for two lanes of the pipeline at 4 097)
  const uint64_t mid_single = o.opt_mid_single > 0 ? (uint64_t)o.opt_mid_single : MID_SINGLE_MIN_DEFAULT;
  // (with one block per window the 12-bit mixed-width pipeline passes it at ~5 600 pairs: mid_parts = 1 keeps that bound)
  const uint64_t mid_single_max = (o.opt_mixed && o.opt_top2 && o.opt_mid_single == 0 && o.opt_mid_parts == 1) ? MID_SINGLE_MAX_MIXED - 1u : MID_NMAX;
  const bool mid = pl.mid = o.opt_mid_single >= 0 && n >= mid_single && n <= mid_single_max && o.opt_c == 0 && wcount == 0 && o.opt_glv <= 0;
  const bool small = pl.small = !mid && n <= small_max && o.opt_c == 0 && wcount == 0;
  // GLV (option "glv" = 1; OFF by default): 2n virtual pairs with 128-bit scalars (+ 1 bit of signed-digit carry) instead of n
  // with 255-bit ones: as many bucket additions, half the windows.  Measured (profiles/r03_glv_msm_on_off.txt) it LOSES at every
  // size from 2^15: the bucket reduction is bound by the depth of its addition chains, not by the number of windows (0.16 ms
  // with 9 windows as with 16); a fifth of the 128-bit magnitudes exceed 2^127, so the signed recoding carries into a ninth
  // window whose entries all land in ONE bucket (the sort's heavy-partition path: 0.09 -> 0.33 ms at 2^20, segmented scan
  // 0.065 -> 0.14); and an entry's x and y come from two arrays (two 32-byte requests instead of one 64-byte one: accumulate
  // 0.82 -> 1.02 ms).  Kept behind the option, with its tests, as the record of the experiment.  The sorted entry packs a
  // 23-bit index, so 2n must fit it.
  const bool glv = pl.glv = o.opt_glv > 0 && !small && wcount == 0 && n >= 2 && 2 * n <= (1ull << 23);
  if (glv) g.n = (u32)(2 * n);
  g.c = mid ? MID_C : (small ? SMALL_C : pick_window_bits(o, n));
  // Mixed window widths (round 5; MsmGeom.top2 = Wb): W = 256 / c windows of which the last Wb = 256 - W c are c + 1 bits wide with 2B
  // buckets, so the windows cover the 256 bit positions exactly -- no carry window, no short top window.  c = 15: 16 + 1 (the
  // "unsigned last window" of the first half of the round is this case), c = 14: 14 + 4, c = 13: 10 + 9, c = 12: 17 + 4, c = 11: 20 + 3,
  // c = 10: 19 + 6; c = 16 is uniform by itself (16 windows of 16 bits).  LDS-sort path only (c >= 10), never for window groups / GLV.
  g.top2 = 0;
  if (g.c >= 10u && g.c <= 15u && !glv && !wcount && !mid && !small && o.opt_top2 && (g.c == 15u || o.opt_mixed)) g.top2 = 256u - (256u / g.c) * g.c;
  g.W = wcount ? wcount : (glv ? 128u / g.c + 1u : (g.top2 ? 256u / g.c : 255u / g.c + 1u));
  g.w0 = w0;
  g.B = 1u << (g.c - 1);
  g.G = (g.W + g.top2) * g.B;
  // up to 2^17 pairs a partition of the sort (<= n entries: one window's) is sorted by ONE block whatever its size (k_fine_sort_part)
  // (c = 16 only above 2^15: the short top window of c = 12 .. 14 is ONE partition of n entries by construction, and one block's two passes
  // over 2^17 entries are 0.15 ms -- measured, profiles/r05_mid_size_ab.txt)
  g.inblock = (o.opt_inblock && (n <= (1u << 15) || ((g.c == 16u || g.top2) && n <= (1u << 17)))) ? 1u : 0u;
  // tools/tune_msm.py sweeps; on the two-lane pipeline 86 entries per thread fill the 3 waves per SIMD exactly once at n = 2^20
  // (profiles/r02_chunk_sweep_two_lanes.txt).  Round 3, at steady clocks (profiles/r03_chunk_sweep_steady_clocks.txt,
  // r03_chunk_length_vs_kernel_events.txt): L = 128 -- one round of TWO waves per SIMD, room for a 144-VGPR wave of the other lane's
  // segmented scan / bucket reduction -- measures 0.99-1.01 ms per step against 1.04 under bench.py, but ONLY there: the HIP events
  // bench.py records around this kernel change the interleaving of the two lanes, and without them (every other caller) L = 128
  // costs 1.19 ms against 1.04.  86 stays; anything between the quantisation points is far worse (L = 120: 1.21).
  // Round 6 (profiles/r06_wave_priority_and_chunk_ab.txt): where another MSM's kernels run BESIDE this accumulation (mode.chained: the pipeline
  // of bpmi_msm_dev_enqueue and of the slices of a large MSM; mode.beside: a synchronous pair from 2^19 pairs) the chunk is the length that makes the
  // accumulation `rounds` rounds of three waves per SIMD, ceil(W n / (64 x 3072 x rounds)), never under 20 entries -- at n = 2^20: 86 for one
  // round (rounds 2 .. 5's choice: every wave slot of the chip taken once, for the whole kernel), 29 for three (the default now).  With one
  // round the other lane's sort and reduction find NO wave slot until the accumulation ends (k_digit_sums 750 us instead of 93, 0.3 ms in
  // every 1.9 without an accumulation running); with three the slots turn over every 0.26 ms, the other lane's kernels become resident
  // beside the accumulation, and -- now that they are resident -- raising their waves' issue priority (option "priority", on by default
  // from this round) lets their dependent chains run at their own speed: 1.043 -> 0.985 ms per step from the chunks alone, -> 0.963 / 0.915
  // (two boxes) with the priority.  Option "rounds" (0 = 3).
  const u32 rounds = o.opt_rounds > 0 ? (u32)o.opt_rounds : 3u;
  const u32 L_lanes = (u32)std::max<uint64_t>(20, ((uint64_t)g.W * g.n + 64ull * 3072 * rounds - 1) / (64ull * 3072 * rounds));
  // One MSM at a time (and the pairs of the IPA): the accumulation as ONE round of three waves per SIMD (3072 waves) from the size
  // where that leaves chunks of 20 entries, one round of two below (a chunk is a chain of dependent additions and every chunk
  // costs a pair of partial records), at most 64.  Powers of two missed the quantisation points:
  // 311 427 pairs at L = 32 are 2 433 waves -- a third round for a fifth of the chip, 0.635 ms against 0.590 at L = 26
  // (profiles/r03_chunk_sweep_wave_quantisation.txt).
  u32 L_one = 64u;
  {
    const uint64_t e_max = (uint64_t)g.W * n;
    auto chunks_for = [&](uint64_t waves) { return (u32)((e_max * 1000 + 64 * waves * 1005 - 1) / (64 * waves * 1005)); };   // 0.5 % over is no extra round
    const u32 l3 = chunks_for(3072), l2 = chunks_for(2048), l1 = chunks_for(1024);
    // Round 5 (profiles/r05_chunk_length_mid_sizes.txt): below ~50 000 pairs the old floor of 8 entries per chunk left 500 .. 1 600 waves
    // -- whatever the count, a SIMD with two waves sets the time -- and the wave counts just under 2 048 win at every size measured
    // (32 768 pairs: L = 5, 1 741 waves, 0.275 ms against 0.293 at L = 8 with 1 088); under three entries per chunk one wave per SIMD
    L_one = l3 >= 20u ? l3 : (l2 >= 3u ? l2 : (l1 < 2u ? 2u : l1));
    if (L_one > 64u) L_one = 64u;
  }
  g.L = o.opt_chunk > 0 ? (u32)o.opt_chunk : ((n >= (1u << 19) && (mode.chained || mode.beside)) ? L_lanes : L_one);
  g.nv = (g.B <= 256u) ? 1u : 4u;                  // partial sums per window handed to the tail
  g.prio = o.opt_prio == 1 ? 15u : (o.opt_prio > 1 ? (u32)(o.opt_prio & 15) : 0u);      // (1 = every stage; 16 + mask = those stages)
  g.fuse = o.opt_fuse ? 1u : 0u;
  // The accumulation by runs (k_accum_runs): the LDS sort's pipeline only (it reuses two of its regions, msm_layout), never GLV.  By default where
  // the buckets are long and even enough for a wave of 64 equally long runs to beat 64 chunks with their boundaries: c = 16 from 2^19 pairs
  // (32 entries per bucket at 2^20), whole MSMs only.  Option "accum_runs" = 2: wherever the LDS sort runs.
  const bool lds_sort = !mid && !small && msm_lds_sort(g.c, g.n);                 // (msm_layout's w.P != 0 for the bucket pipeline)
  g.runs = 0;
  if (lds_sort && !glv && g.G >= 2048u && (o.opt_accum_runs == 2 || (o.opt_accum_runs == 1 && g.c == 16u && !wcount && n >= (1u << 19)))) g.runs = 1;
  return pl;
}
// The longest run the accumulation by runs takes: twice the mean run length ceil(n W / G) plus 64.  A thread adds its run alone, so the kernel
// lasts as long as the longest one: uniform digits (Poisson around the mean) never reach the cap, and every skewed input -- equal scalars, bit
// vectors, a few distinct values: one bucket with a large part of a window's n entries -- passes it by orders of magnitude.
static inline u32 msm_runs_cap(const BpmiOptions &o, const MsmGeom &g) {
  if (o.opt_accum_runs_cap > 0) return (u32)o.opt_accum_runs_cap;
  const uint64_t mean = ((uint64_t)g.n * g.W + g.G - 1) / g.G;
  return (u32)std::min<uint64_t>(2 * mean + 64, 1ull << 30);
}
// length classes of the run table for that cap (class = min(length, classes - 1)) and its blocks
static inline u32 msm_runs_bins(u32 cap) { return std::min<u32>(cap, RUN_BINS - 1u) + 1u; }
static inline u32 msm_runs_blocks(const MsmGeom &g) { return (g.G + RUN_SLICE - 1u) / RUN_SLICE; }

struct MsmWs {
  u32 *glv_sub, *glv_bx;      // GLV: 2n x 16 B magnitudes, n x 32 B beta x
  unsigned char *glv_neg;     // GLV: 2n sign bytes
  u32 *dig, *hist, *off, *cursor, *bsum, *sidx, *buckets, *chunk_key, *coarse_hist, *coarse_off, *coarse_cursor;
  unsigned short *dig16;      // path 2: recoded digits, window-major
  unsigned char *negs;        // path 2: 1 = the scalar was replaced by q - s
  u32 P;          // partitions of sort path 2 (0 = path 1)
  u32 *rec_key[2], *rec_pt[2];
  u32 *D, *E, *F, *out;
  u32 *run_order, *run_counts, *run_flags;     // the run table (MsmGeom.runs): in `cursor`, `hist` and the spare words of `coarse_hist`
  size_t total;
  u32 nscan_blocks, rec0_max, nchunks;
};
// the workspace of one MSM at `base` (nullptr: the sizing pass, only w.total and the counts mean anything)
static inline void msm_layout(const MsmGeom &g, MsmWs &w, char *base, bool glv = false) {
  size_t o = 0;
  auto take = [&](size_t bytes) { char *p = base ? base + o : nullptr; o += align_up(bytes, 256); return (u32 *)p; };
  w.glv_sub = take(glv ? 16ull * g.n : 0);               // g.n = virtual pairs
  w.glv_bx = take(glv ? 16ull * g.n : 0);
  w.glv_neg = (unsigned char *)take(glv ? g.n : 0);
  const size_t nW = (size_t)g.n * g.W;
  w.nscan_blocks = (u32)((g.G + SCAN_TILE - 1) / SCAN_TILE);
  w.nchunks = (u32)((nW + g.L - 1) / g.L);                  // threads of k_accum_l0
  w.rec0_max = 2u * (g.fuse ? (w.nchunks + 63u) / 64u : w.nchunks);
  // second-level segscan buffer sizing relies on this: every level after the first has at most rec1_max records (R shrinks monotonically)
  const u32 rec1_max = 2 * ((w.rec0_max + 255) / 256);
  w.P = msm_lds_sort(g.c, g.n) ? (g.G >> 8) : 0;            // partitions of sort path 2; 0 = path 1
  w.hist = take(4ull * g.G);                 // path 1 only
  w.off = take(4ull * (g.G + 1));
  w.cursor = take(4ull * g.G);               // path 1 only
  w.bsum = take(4ull * (w.nscan_blocks + 1));
  w.coarse_hist = take(4ull * COARSE_HIST_WORDS);
  w.coarse_off = take(4ull * (PART_MAX + 1));
  w.coarse_cursor = take(4ull * (PART_MAX + 1));
  w.dig = take(4ull * nW);                   // path 1: digits; path 2: partitioned entries
  w.sidx = take(4ull * nW);
  w.dig16 = (unsigned short *)take(w.P ? 2ull * nW : 0);
  w.negs = (unsigned char *)take(w.P ? g.n : 0);
  w.chunk_key = take(4ull * (w.nchunks + 1));
  w.buckets = take(4ull * XYZZ_WORDS * g.G);
  w.rec_key[0] = take(4ull * w.rec0_max);
  w.rec_pt[0] = take(4ull * XYZZ_WORDS * w.rec0_max);
  w.rec_key[1] = take(4ull * rec1_max);
  w.rec_pt[1] = take(4ull * XYZZ_WORDS * rec1_max);
  w.D = take(4ull * XYZZ_WORDS * g.W * (g.B > 256u ? (1u << ((g.c + 1u) / 2u)) + (1u << (g.c / 2u)) : 1u));   // stage-1 digit sums
  w.E = take(4ull * XYZZ_WORDS * g.W * 4);
  w.F = take(4ull * XYZZ_WORDS * g.W * 64);       // k_digit_final_spread: 16 sums per (window, array)
  w.out = take(64);
  // the run table is built when the sort is over, in two of its regions that are dead by then: order[] (at most G bucket keys) in `cursor`,
  // the per-block counts (msm_runs_blocks x at most RUN_BINS words <= G from 2048 buckets) in `hist`
  w.run_order = w.cursor; w.run_counts = w.hist; w.run_flags = w.coarse_hist;
  w.total = o;
}

static inline u32 msb_index(u32 v) { u32 k = 0; while ((2u << k) <= v) k++; return k; }     // floor(log2 v), v >= 1
// lanes per sum for `epl` elements per lane: a sum lives in ONE wave, so the group is widened to the largest size that keeps the same
// number of sums per wave (12 lanes -> 5 sums per wave; 13 .. 16 lanes -> 4)
static inline void digit_group(DigitJob &j, u32 elements, u32 epl) {
  u32 lanes = (elements + epl - 1u) / epl;
  if (lanes > 64u) lanes = 64u;
  if (lanes < 1u) lanes = 1u;
  j.gpw = 64u / lanes;
  j.glanes = 64u / j.gpw;
  if (j.glanes > elements) j.glanes = elements ? elements : 1u;
}
static inline u32 digit_job_waves(const DigitJobs &J, u32 k) {
  const uint64_t sums = (uint64_t)J.j[k].cnt * J.j[k].nsums;
  return (u32)((sums + J.j[k].gpw - 1u) / J.j[k].gpw);
}
static inline u32 digit_job_blocks(const DigitJobs &J, u32 k) { return (digit_job_waves(J, k) + 3u) / 4u; }
// the two jobs (by lo, by hi) that split every array [in_off .. in_off + N) of `cnt` arrays at bit s;
// results at out_off (2^s - 1 sums) and behind them (N >> s sums)
static inline DigitJobs digit_jobs2(u32 cnt, u32 in_off, u32 in_stride, u32 N, u32 s, u32 out_off, u32 out_stride, u32 epl) {
  DigitJobs J;
  memset(&J, 0, sizeof(J));
  J.njobs = 2;
  for (u32 type = 0; type < 2; type++) {
    DigitJob &j = J.j[type];
    j.cnt = cnt;
    j.in_off = in_off; j.in_stride = in_stride; j.N = N; j.s = s; j.type = type;
    j.nsums = type ? (N >> s) : ((1u << s) - 1u);
    digit_group(j, type ? (1u << s) : ((N - 1u) >> s) + 1u, epl);
    j.out_off = out_off + (type ? (1u << s) - 1u : 0u); j.out_stride = out_stride;
  }
  J.j[0].blk0 = 0;
  J.j[1].blk0 = digit_job_blocks(J, 0);
  return J;
}
static inline DigitJobs digit_jobs_concat(const DigitJobs &a, const DigitJobs &b) {
  DigitJobs J = a;
  u32 blk = a.j[1].blk0 + digit_job_blocks(a, 1);
  for (u32 k = 0; k < 2; k++) { J.j[2 + k] = b.j[k]; J.j[2 + k].blk0 = blk; blk += digit_job_blocks(b, k); }
  J.njobs = 4;
  return J;
}

// The bucket reduction of a geometry with more than 256 buckets per window (g.B > 256; smaller windows take one launch of
// k_window_weighted_small and need no plan: njobs = 0, to.nv = 1).  Bucket index b in [1, B], B = 2^(c-1):  b = hi 2^s0 + lo, then
// each digit again in two -- the four digits' bit offsets are the tail's `to`.
struct MsmReducePlan {
  DigitJobs j1;            // stage 1 (k_digit_sums): buckets -> D0[1..N0], D1[1..N1] per window, `grid1` blocks
  DigitJobs j2, j2top;     // stage 2 + finish: the windows with B buckets, the wide ones (njobs = 0 without them)
  u32 grid1, top_w;        // top_w: the first wide window (0xFFFFFFFF: none)
  TailOffs to;
};
static inline MsmReducePlan msm_reduce_plan(const MsmGeom &g, const BpmiOptions &o) {
  MsmReducePlan r{};
  r.to.nv = 1;
  r.top_w = 0xFFFFFFFFu;
  if (g.B <= 256u) return r;
  const u32 s0 = g.c / 2u, N0 = (1u << s0) - 1u, N1 = g.B >> s0;          // stage-1 arrays: D0[1..N0], D1[1..N1]
  const u32 t0 = (s0 + 1u) / 2u, t1 = (msb_index(N1) + 1u) / 2u;          // stage-2 splits
  const u32 stride1 = N0 + N1;
  // stage 1: as many elements per lane as keep about one wave on every SIMD (16 at c = 16 with all 16 windows: measured
  // best of 4 / 8 / 12 / 16 there; fewer buckets -- smaller c, a window group of a split MSM -- get shorter chains
  // instead of idle SIMDs); stage 2 + the finish are pure latency: one element per lane, 16-lane butterflies, one launch
  const u32 Wr = g.W - g.top2;                       // windows with B buckets
  // the wide windows (mixed widths, g.top2 of them): arrays of 2B buckets behind the others, split like windows of c + 1 bits (their D sums
  // fit the per-window slot of w.D: 2^((c+1)/2) + 2^(c/2) records)
  const u32 Bt = 2u * g.B, s0t = (g.c + 1u) / 2u, N0t = (1u << s0t) - 1u, N1t = Bt >> s0t;
  const u32 t0t = (s0t + 1u) / 2u, t1t = (msb_index(N1t) + 1u) / 2u;
  const u32 d_top = Wr * stride1, stride1t = N0t + N1t;      // first D record of the wide windows, and their records per window
  auto stage1 = [&](u32 epl, DigitJobs &j) -> u32 {  // the jobs for `epl` elements per lane; returns their waves
    j = digit_jobs2(Wr, 0, g.B, g.B, s0, 0, stride1, epl);
    u32 waves = digit_job_waves(j, 0) + digit_job_waves(j, 1);
    if (g.top2) {
      DigitJobs jt = digit_jobs2(g.top2, Wr * g.B, Bt, Bt, s0t, d_top, stride1t, epl);
      waves += digit_job_waves(jt, 0) + digit_job_waves(jt, 1);
      j = digit_jobs_concat(j, jt);
    }
    return waves;
  };
  if (o.opt_epl > 0) stage1((u32)o.opt_epl, r.j1);
  else if (o.opt_reduce_fit) {
    // the fewest elements per lane whose waves fit the chip's 1 024 SIMDs at one each: a wave alone on its SIMD already runs at
    // 86 % of the multiply-add pipe, so a SIMD with two takes twice as long (c = 15 with 16-lane sums: 1 148 waves, 124 SIMDs doubled,
    // no faster than c = 16; with 12-lane sums, five to a wave: 931)
    u32 epl = 2;
    while (epl < 64u && stage1(epl, r.j1) > 1024u) epl++;
  } else {
    u32 epl = (u32)(((uint64_t)g.G) >> 15);
    stage1(epl < 2u ? 2u : (epl > 16u ? 16u : epl), r.j1);
  }
  // stage 2: D0 -> (D00, D01), D1 -> (D10, D11), each <= 16 sums of <= 16 elements, and E[a][r] = sum_d d * D..[d]
  r.j2 = digit_jobs_concat(digit_jobs2(Wr, 0, stride1, N0, t0, 0, 64, 1), digit_jobs2(Wr, N0, stride1, N1, t1, 0, 64, 1));
  r.to.nv = 4; r.to.off[0] = 0; r.to.off[1] = t0; r.to.off[2] = s0; r.to.off[3] = s0 + t1;
  if (g.top2) {
    r.j2top = digit_jobs_concat(digit_jobs2(g.top2, d_top, stride1t, N0t, t0t, 0, 64, 1), digit_jobs2(g.top2, d_top + N0t, stride1t, N1t, t1t, 0, 64, 1));
    r.to.top = g.top2; r.to.top_off[0] = 0; r.to.top_off[1] = t0t; r.to.top_off[2] = s0t; r.to.top_off[3] = s0t + t1t;
    r.top_w = Wr;
  }
  r.j1.prio = g.prio & PRIO_SUMS;
  r.j2.prio = r.j2top.prio = g.prio & PRIO_FINISH;
  r.grid1 = r.j1.j[r.j1.njobs - 1].blk0 + digit_job_blocks(r.j1, r.j1.njobs - 1);
  return r;
}

// ---- large inputs as slices of the size where the engine peaks (round 6) -------------------------------------------------------
// The reference's multiexp takes any N (/root/reference/src/pippenger/pippenger.py:22-61) and its verifier calls it with 2n + 1 pairs
// (/root/reference/src/innerproduct/inner_product_verifier.py:134-139: 2^21 + 1 at config C3's size).  One MSM of more than ~2^20 pairs
// runs BELOW the 2^20 rate here (7.75-8.3 x 10^8 pairs/s at 2^21 .. 2^24 against 1.0 x 10^9, profiles/r03_msm_big_n.txt): its 64-byte
// gathers, once per window, no longer fit the Infinity Cache, and one MSM at a time leaves the chip to the sort and to the bucket
// reduction for 0.3 ms per MSM.  So an input of slice_min (1.625 slice_n) pairs or more is cut into K = ceil(total / (slice_n 17/16)) equal slices,
// which run as the two-deep pipeline of bench.py's headline (lanes 0 / 1, the accumulations chained): the sort and the reduction of one
// slice beside the accumulation of the other, the host tail of slice k under the kernels of slice k + 1.  The slices' affine results
// are added on the host (XYZZ, one inversion).  Options "slice_n" (0 = 2^20; -1 = never slice below the sort's 2^23 limit) and
// "slice_min" (0 = default).  Inputs with half-block selection (the IPA's deferred folds: msm_run_pair) are never sliced.
#define SLICE_N_DEFAULT (1u << 20)
#define SLICE_N_LIMIT (1u << 23)          // the packed sort entry holds a 23-bit pair index
static inline bool segs_dense(const Segs &s) { return s.hlog[0] >= 32u && s.hlog[1] >= 32u && s.hlog[2] >= 32u && !s.glv_sub; }
// the logical pairs [lo, lo + cnt) of a dense `s`
static inline Segs segs_slice(const Segs &s, uint64_t lo, uint64_t cnt) {
  Segs r = segs_init();
  u32 k = 0;
  uint64_t base = 0;
  for (int i = 0; i < 3; i++) {
    const uint64_t a = std::max<uint64_t>(lo, base), b = std::min<uint64_t>(lo + cnt, base + s.n[i]);
    if (b > a) { r.pts[k] = s.pts[i] + 16ull * (a - base); r.sc[k] = s.sc[i] + 8ull * (a - base); r.n[k] = (u32)(b - a); k++; }
    base += s.n[i];
  }
  r.total = (u32)cnt;
  return r;
}
// slice k of a total cut into slices of `per` = ceil(total / K) pairs: the pairs [lo, lo + cnt)
struct MsmSlice { uint64_t lo, cnt; };
static inline MsmSlice msm_slice(uint64_t total, uint64_t per, uint64_t k) { return MsmSlice{k * per, std::min<uint64_t>(per, total - k * per)}; }
static inline uint64_t msm_slice_count(const BpmiOptions &o, const Segs &segs) {
  // (forced window bits, window groups, half-block selections: ONE MSM whatever its size -- beyond 2^23 pairs on the global-atomic sort)
  if (!segs_dense(segs) || o.opt_c || o.opt_split) return 1;
  const uint64_t slice_n = o.opt_slice_n < 0 ? SLICE_N_LIMIT : std::min<uint64_t>(o.opt_slice_n ? (uint64_t)o.opt_slice_n : SLICE_N_DEFAULT, SLICE_N_LIMIT);
  const uint64_t slice_min = o.opt_slice_n < 0 ? SLICE_N_LIMIT + 1 : (o.opt_slice_min ? (uint64_t)o.opt_slice_min : slice_n + slice_n / 2 + slice_n / 8);      // (measured crossover of one MSM against two slices: ~1.65 x 2^20 pairs)
  if (segs.total < slice_min && segs.total <= SLICE_N_LIMIT) return 1;
  const uint64_t cap = std::min<uint64_t>(slice_n + slice_n / 16, SLICE_N_LIMIT);       // a slice may be a sixteenth over (2^21 + 1 pairs: two slices, not three)
  return std::max<uint64_t>(2, (segs.total + cap - 1) / cap);
}
