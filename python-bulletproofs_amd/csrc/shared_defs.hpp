// shared_defs.hpp -- part of libbpmi; plain C++17 (no HIP), also compiled for the host by tests/csrc_host.
// What the kernels, the host orchestration and the host-only planners (msm_plan_host.hpp, rp_batch_plan_host.hpp) all read: the
// engine's options, the multi-segment input descriptor and the sizing constants of the MSM and of the batch verifier.  One
// definition of each.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/bpmi.h"
#include "curve.hpp"

using bpmi::u32;
using bpmi::TailOffs;

#define XYZZ_WORDS 36
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
// k = the smallest one with 2^k >= n; true when n is that power of two
static inline bool log2_exact(uint64_t n, u32 &k) { k = 0; while ((1ull << k) < n) k++; return n && (1ull << k) == n; }

// up to three (points, scalars) segments presented as one logical array, so that
// e.g. L = <a_lo, g_hi> + <b_hi, h_lo> + cl*u is ONE MSM without any gather/concat
// (the reference concatenates Python lists: src/utils/commitments.py:13)
struct Segs {
  const u32 *pts[3];
  const u32 *sc[3];
  u32 n[3];
  u32 total;
  // Optional half-block selection per segment: with hlog[s] = h < 32 the logical element j of
  // segment s is the physical element ((j >> h) << (h + 1)) | (phase[s] << h) | (j & (2^h - 1)),
  // i.e. only the lower (phase 0) or upper (phase 1) half of every block of 2^(h+1) elements.
  // The deferred-fold MSMs of the IPA use it to skip the half of the scalars that is zero by
  // construction.  hlog[s] >= 32: dense (the default, set by segs_init).
  u32 hlog[3];
  u32 phase[3];
  // GLV (scalar.hpp glv_split; prepared per MSM by k_glv_prepare, csrc/msm_kernels.hpp): when glv_sub is set the MSM runs over
  // 2 * total VIRTUAL pairs -- virtual pair 2i is (P_i, |k1_i|), 2i + 1 is (lambda P_i, |k2_i|) -- with 128-bit magnitudes
  // glv_sub[4 v ..] and signs glv_neg[v]; lambda P_i = (beta x_i, y_i), the x coordinates precomputed in glv_bx[8 i ..].
  const u32 *glv_sub;
  const unsigned char *glv_neg;
  const u32 *glv_bx;
};
static inline Segs segs_init() {
  Segs s;
  memset(&s, 0, sizeof(s));
  s.hlog[0] = s.hlog[1] = s.hlog[2] = 0xFFu;
  return s;
}
// One dense array: logical pair i is physical pair i of segment 0 -- the point of a sort entry is pts[0] + 16 * index with no segment
// walk and no half-block remap (k_accum_runs<true>).  Never with GLV: its entries index virtual pairs.
static inline bool segs_one_dense(const Segs &s) {
  return s.total != 0 && s.n[0] == s.total && s.n[1] == 0 && s.n[2] == 0 && s.hlog[0] >= 32u && !s.glv_sub;
}

// ---- sizing constants of the MSM (the kernels they belong to: msm_kernels.hpp) ------------------------------------------------
// MsmGeom.prio is a mask of the stages whose kernels raise their waves' issue priority (raise_priority, msm_kernels.hpp):
#define PRIO_SORT 1u          // recoding, partition, level B of the sort
#define PRIO_SCAN 2u          // segmented scan over the partial records
#define PRIO_SUMS 4u          // stage 1 of the bucket reduction (throughput-bound: 2^20 general additions)
#define PRIO_FINISH 8u        // the reduction's finish on quads of lanes (latency-bound chains)
#define PART_MAX 2048          // sort path 2: W * (B / 256) <= 2048 partitions for every c in [10, 16]
#define COARSE_HIST_WORDS (PART_MAX + 192)     // the partition counts, the any_heavy flag (+0), the tickets of the last-block fusions (+1, +2) and of
                                               // k_digit_final_spread (+8 .. +8 + 4 W), padded to whole 256-byte lines
#define FINE_TILE 4096           // entries per tile of the sort's heavy-partition kernels
// the run table of the accumulation by runs (k_runs_hist / k_runs_scatter / k_accum_runs, msm_kernels.hpp): its flag and count live in the spare
// words of coarse_hist behind the tickets, zeroed by the sort's memset
#define RUN_FLAG_WORD (PART_MAX + 3)     // long_run: some run is longer than the cap -> the chunked accumulation and the segmented scan do the work
#define RUN_COUNT_WORD (PART_MAX + 4)    // nruns: non-empty buckets
#define RUN_BINS 1024u           // length classes of the counting sort; runs of RUN_BINS - 1 entries or more share the last one (in bucket order)
#define RUN_SLICE 4096u          // buckets per block of the two table kernels (128 blocks at 2^19 buckets, 16 buckets per thread); a multiple of 256
#define SCAN_PER_THREAD 16
#define SCAN_TILE (256 * SCAN_PER_THREAD)
#define SMALL_C 8                // window bits of k_msm_small
#define MID_C 7                  // window bits of k_msm_mid
#define MID_NMAX 8448            // pairs per MSM: the digit and entry arrays live in LDS (139 KB of the 160 KB a gfx950 CU has: this kernel does not build for earlier CDNA parts)
#define GROUP_LIGHT_THREADS 256  // the light shape of k_msm_group (small groups: 52 KB of LDS) ...
#define GROUP_LIGHT_NMAX 512     // ... and the pairs per group it takes

// ---- sizing constants of the batch verifier (the kernels they belong to: rp_batch_kernels.hpp) ---------------------------------
// Four waves per group of `lanes` proofs, one per ROLE (see the head of rp_batch_kernels.hpp)
#define RP_ROLES 4
// A wire proof longer than this is invalid (on the device and in the host twin, rp_batch_host.hpp): it bounds the transposed
// array.  A 64-bit proof is 2.6 KB, the largest shape the format allows (k = 16) under 8 KB.
#define RP_MAX_PROOF_BYTES 32768u
#define CTX_SLOTS(k_, m_) (2u + 3u * (k_) + (m_))      // context slots of one proof (the CTX_* indices, rp_batch_kernels.hpp)
#define RP_MIXED_MAX_CLASSES 64   // classes of one mixed batch (bpmi_rp_batch_verify_mixed_dev)
#define RP_MIXED_UNIT_STRIDE 256  // bytes of one slot of a mixed batch's unit table (rpd::MixedUnit, rp_batch_kernels.hpp)
#define RP_UPLOAD_SLICES 4       // a batch of 4 096 proofs or more is uploaded in up to this many slices (ctx->ev_slice)

// ---- options (bpmi_set_option, include/bpmi.h); bpmi_ctx inherits them, so ctx->opt_c is this opt_c ----------------------------
struct BpmiOptions {
  int opt_c = 0;        // window bits, 0 = auto
  int opt_tail = 0;     // 0 auto, 1 device, 2 host
  int opt_prio = 1;     // MSM: the stages around the accumulation raise their waves' issue priority (s_setprio): 0 none, 1 all (default from round 6: beside a multi-round
                        // accumulation it is a gain, profiles/r06_wave_priority_and_chunk_ab.txt; round 3 measured a loss beside the one-round kernel), 16 + mask = those PRIO_* stages
  int opt_hist_threads = 0, opt_hist_blocks = 0;     // k_coarse_hist launch shape (0 = default)
  int opt_quad = 1;     // bucket reduction's finish with four-lane point additions (k_digit_final_quad); 0 = one lane per point
  int opt_mulb = 1;     // bpmi_ec_mul_batch: 1 = GLV + fixed signed windows over affine odd multiples (n >= MULB_MIN_N), 0 = the bit-serial ladder
  int opt_chunk = 0;    // entries per thread in k_accum_l0, 0 = auto
  int opt_small = 0;    // largest n handled by the one-launch small-MSM kernel (0 = default, -1 = never)
  int opt_fold_wnaf = 2;     // the IPA's 16-way generator fold: 2 = width-4 NAF of the coefficients' GLV halves over affine tables of odd multiples, 1 = of the whole coefficients, 0 = plain NAF ladder
  int opt_rp_only_role = -1; // profiling only: run one role of the batch preparation kernel (the call then reports proof 0 as bad)
  int opt_glv = 0;           // MSM on GLV-split scalars (an experiment that lost, profiles/r03_glv_msm_on_off.txt): 0 / -1 = never (default), 1 = whenever the bucket pipeline runs
  int opt_rp_prio = 1;       // batch preparation: its kernels (expander, roles, elements) raise their waves' issue priority: 0 never, 1 on wire formats 1 and 2 (square roots run beside them), 2 always
  int opt_rp_slices = 0;     // batch preparation: uploads of a batch of >= 4096 proofs (1 .. 4); 0 = 4 for formats 1 and 2 (a slice's points are decoded beside the next upload), 1 for format 3
  int opt_rp_overlap = 1;    // batch preparation: point decoding on the second lane beside the preparation kernels (0: behind them; measurements)
  int opt_rp_rows = 0;       // batch preparation: proofs per launch (0 = as many as fit ~256 MB of contribution cells)
  int opt_rp_lanes = 0;      // batch preparation kernel: proofs per wave (0 = chosen from the batch size)
  int opt_epl = 0;           // bucket reduction stage 1: elements per lane (0 = default 16)
  int opt_tail_thread = 1;   // a synchronous PAIR of MSMs: the host tail of the second one runs on the ctx's helper thread beside the first one's (0: one after the other)
  int opt_pair_chain = 0;    // a synchronous pair of LARGE MSMs: 1 = their accumulate kernels chained as in the asynchronous pipeline (A/B; round 3 measured it slower)
  int opt_mid_min = 0;       // a pair of MSMs runs as one launch of k_msm_mid from this many pairs in the larger one (0 = default 1536, -1 = never)
  int opt_mid_single = 0;    // a single MSM runs on k_msm_mid from this many pairs (0 = default 2560, -1 = never)
  int opt_pair1 = 1;         // a pair of SMALL MSMs (bpmi_msm2, the L / R of an inner-product round) as one launch sequence on one stream (0: two lanes)
  int opt_fuse = 1;          // k_accum_l0 folds a wave's partial records itself (0: two records per thread, the round-3 path; A/B and tests)
  int opt_spin_wait = 0;     // polls of an event / stream before sleeping in the runtime (see wait_event; measured: no gain, off)
  int opt_async_lanes = 0;   // 1: slot 1 of the asynchronous MSM pair runs on the second lane
  int opt_split = 0;    // 1: one MSM as two window groups, one per lane (measured: +5 % at 2^20, -8 % at 2^19; off)
  int64_t opt_ipa_big = 0;   // base length from which the IPA folds generators 16-way (0 = default 2^18)
  int opt_ipa_step = 0;      // short inner-product vectors: fold + coefficient tables + the next round's dots and scalars in ONE launch (k_ipa_small_step).
                             // Measured (profiles/r04_C3_small_step_ab.txt): the one block takes 60 us where the four launches it replaces take 25 + gaps:
                             // 25.1-25.3 ms per proof against 24.5.  OFF; kept with its tests (tools/fuzz_ops.py draws it)
  int opt_fold_shared = 1;   // the product fold of a state without per-generator scales: shared GLV halves, two terms per thread (0: per-lane products)
  int64_t opt_ipa_small = 0; // logical length at which smaller bases are folded through products (0 = default 4096, 1 = never)
  int opt_ipa_fixed = 0;     // 1: the generator arrays of bpmi_ipa_create_dev are deployment constants: the fold's tables of their odd multiples are kept between proofs
  int opt_direct = 1;                   // the last kernel of an MSM writes its result into the slot's page-locked host buffer (0: workspace + copy)
  int opt_pair_phases = 0;              // 1: a synchronous pair of MSMs queues both sorts before either accumulation (measured neutral: profiles/r04_C3_pair_phases_ab.txt)
  int opt_graph = 0;                    // 1: replay an MSM's launch sequence as a HIP graph when the same call comes again
  // round 5 (the mid-size floor; every one on by default, 0 = the round-4 path for A/B runs and tests)
  int opt_mid_parts = 0;                // k_msm_mid: blocks per window (0: three from 3 000 pairs, else one; 1 .. 4 forced)
  int opt_mixed = 1;                    // window bits 10 .. 14 as mixed widths c / c + 1 covering 256 bits exactly (15 always does, under opt_top2)
  int opt_top2 = 1;                     // c = 15: 17 windows, the last one unsigned with 2B buckets (0: 18 windows, the last one a carry window)
  int opt_reduce_fit = 1;               // stage 1 of the bucket reduction: elements per lane chosen so that its waves fit the SIMDs at one each
  int opt_final_spread = 3;             // the bucket reduction's finish: 0 one 16-wave block per array, 1 one-wave blocks + tickets, 2 / 3 two launches (include/bpmi.h)
  int opt_inblock = 1;                  // n <= 2^17: the sort's level B handles partitions of any size itself, the two heavy-tile launches are skipped
  int opt_prover_tw = 0;                // bpmi_rp_prover_create: window bits of the fixed-base tables (0 = default by size, rp_prove_plan_host.hpp; 4 .. 16)
  int opt_prover_job_lanes = 0;         // bpmi_rp_prove_batch: lanes per multi-scalar multiplication: 0 by the job count (rpp_job_lanes_log2), 16, 64
  int opt_validate = 1;                 // on-curve check of the points a caller hands in: 0 never, 1 the host-pointer entry points (default), 2 the synchronous _dev ones too
  int opt_histscan = 0;                 // 1: the scan of the sort's partition counts runs in the block of k_coarse_hist that flushes last.  LOST (profiles/r05_last_block_fusions_ab.txt):
                                        // the device-scope fence every block needs writes its XCD's L2 back behind 33 MB of digit codes -- +60 us at 2^20, +16 us at 2^16.  Off; kept with its tests
  int opt_segfuse = 0;                  // 1: the segmented scan's last level runs in the block that finishes the level before it last.  No gain one MSM at a time, and the fence costs
                                        // two MSMs in flight 3 % (the other lane's dirty bucket lines are written back with it).  Off; kept with its tests
  // round 6
  int opt_slice_n = 0;                  // an MSM of more than slice_min pairs runs as slices of about this many, two in flight (0 = 2^20, -1 = only beyond the sort's 2^23 limit; msm_plan_host.hpp)
  int opt_slice_min = 0;                // ... the size from which it does (0 = default: 1.25 x slice_n)
  int opt_pair_sched = 0;               // 1: a synchronous pair of large MSMs as both sorts, then the accumulations one after the other (msm_run_pair).  Measured neutral
                                        // (profiles/r06_C3_pair_sched_ab.txt): off
  int opt_prover_wire = 2;              // bpmi_rp_prove_batch: the wire format of the proofs it returns, 2 or 3 (3: with the points' y coordinates, rp_wire_v2_host.hpp)
  int opt_prover_split = 0;             // bpmi_rp_prove_batch: 1 = a batch of 4 096 proofs or more as two halves on two lanes, N > 1 = from 2 N proofs (rp_prove_host.hpp).
                                        // Measured: 19.7-19.9 ms against 19.4-19.6 for 2^14 proofs (profiles/r06_batch_prover_table_bits.txt): off
  int opt_rounds = 0;                   // rounds of three waves per SIMD of an accumulation that shares the chip with another MSM's kernels (0 = 3; msm_plan_host.hpp)
  int opt_pair_rounds = 0;              // 1: a synchronous pair of large MSMs keeps round 5's one-round chunks (A/B)
  int opt_accum_chain = 1;              // experiment: 0 = the asynchronous pipeline's accumulations are NOT ordered after each other (the lanes run free)
  int opt_accum_stream = 0;             // experiment: the chained pipeline's accumulations on one low-priority stream of their own (msm_host.hpp)
  int opt_lane_prio = 0;                // experiment: queue priority of lanes 1 / 2 created AFTER the option is set (0 default, -1 high, 1 low)
  int opt_accum_runs = 1;               // the accumulation as one length-sorted bucket run per thread (k_accum_runs): 0 never, 1 where it pays (msm_pick_geometry), 2 wherever the LDS sort runs (tests)
  int opt_accum_runs_cap = 0;           // ... the run length beyond which an MSM falls back to the chunked accumulation (0 = the rule, msm_runs_cap; tests force either side)
  // bulk hash to the curve (h2c_host.hpp)
  int opt_h2c_plain = 0;                // 1: one message per lane with a loop per lane (k_h2c_plain) at EVERY size, not only where a lane has one message anyway
  int opt_h2c_per_lane = 0;             // 1 .. 64: k_h2c_queue with that many messages per lane of a wave's span (0 = by the call's size, h2c_span)
  // batched MSM over shared points (msm_batch_plan_host.hpp)
  int opt_msm_batch_route = 0;          // 0 by the sizes, 1 / 2 / 3 forces the light shape / the k_msm_mid shape / the loop of single MSMs (tests, A/B runs)
  int opt_msm_batch_vecs = 0;           // vectors per launch (0 = as many as keep a launch's window sums within 256 MB)
};
