// bpmi.hip -- libbpmi.so: MSM + inner-product-argument engine for MI355X (gfx950).
// C-ABI in include/bpmi.h; design notes in DESIGN.md.
//
// MSM pipeline (replaces Pippenger.multiexp, /root/reference/src/pippenger/pippenger.py:22-94,
// by the signed-digit bucket method; the result -- a canonical affine point -- is
// schedule independent, so it is bit-identical to the reference's subset-table schedule):
//   sort            (window, bucket) counting sort of (point index, sign):
//                   n >= 2^16 (window bits >= 10): k_coarse_hist / k_partition / k_fine_sort_part --
//                   a two-level radix partition whose histograms and ranks live in LDS
//                   (global atomics only reserve one range per tile and partition; level B
//                   sorts one partition per block and writes one contiguous range);
//                   smaller n: k_digits_hist / k_scatter with global atomics
//   k_scan_*        exclusive scans of the (coarse) histograms -> run offsets
//   k_accum_runs    (16-bit windows from 2^19 pairs) every thread adds ONE whole bucket run, the buckets in order
//                   of their run length (k_runs_hist / k_runs_scatter: a counting sort of the buckets); a
//                   flag on the device hands MSMs with a long run to the next two kernels.  <true>: one
//                   dense array, the point of an entry fetched without the segment walk; the first two
//                   entries of a run stand in front of the loop (the second: affine + affine, xyzz_mmadd)
//   k_accum_l0      every thread adds exactly L sorted entries (perfectly balanced for
//                   ANY digit distribution); runs that end inside a chunk go to their
//                   bucket, the first/last run of a chunk become partial records
//   k_segscan       block-wide segmented scan over partial records, 256 -> 2 per block,
//                   repeated until one block is left
//   k_digit_sums / k_digit_final       sum_b b*B[w][b]: the bucket index split in two digits, twice
//                   twice (2 additions per element, sub-wave groups, shuffle butterflies),
//                   then 16-term suffix scans; k_window_weighted_small for <= 256 buckets
//   k_msm_small     n <= 4096: digit multiples per thread + butterfly sums (latency path)
//   tail            O(256) sequential doublings: window combine + to-affine
//                   (host thread on 4x64-bit limbs, host_tail.hpp, or the one-lane device
//                   kernel k_tail; same Horner chain)
// This file: the C-ABI entry points.  What every one of them relies on: the options (one table, options_host.hpp) and the on-curve check of
// caller-supplied points (one object, point_check_host.hpp).  The inner-product prover (the IPA state object, deferred generator folding) is ipa_host.hpp,
// included below where its section stood; the batch verifier of inner-product proofs is ipa_batch_host.hpp, behind it.
// Kernels and host orchestration live in the *.hpp files included below (one translation unit).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "../../include/bpmi.h"
#include "curve.hpp"
#include "field.hpp"
#include "scalar.hpp"

using namespace bpmi;

#define BPMI_VERSION 100

#include "shared_defs.hpp"
#include "options_host.hpp"
#include "msm_plan_host.hpp"
#include "rp_batch_plan_host.hpp"
#include "rp_mixed_plan_host.hpp"
#include "rp_group_mixed_plan_host.hpp"
#include "rp_prove_plan_host.hpp"
#include "rp_prove_mixed_plan_host.hpp"
#include "ipa_prove_plan_host.hpp"
#include "ipa_prove_mixed_plan_host.hpp"
#include "ipa_batch_plan_host.hpp"
#include "ipa_mixed_plan_host.hpp"
#include "ipa_packed_plan_host.hpp"
#include "ipa_packed_mixed_plan_host.hpp"
#include "ipa_wire_plan_host.hpp"
#include "ipa_group_plan_host.hpp"
#include "ipa_group_mixed_plan_host.hpp"
#include "msm_batch_plan_host.hpp"
#include "msm_fixed_plan_host.hpp"
#include "context.hpp"
#include "device_util.hpp"
#include "msm_kernels.hpp"
#include "msm_fixed_kernels.hpp"
#include "fold_ops_host.hpp"
#include "point_kernels.hpp"
#include "point_check_host.hpp"
#include "svector_batch.hpp"
#include "svector_mixed.hpp"
#include "scalar_kernels.hpp"
#include "ipa_mixed_kernels.hpp"
#include "host_tail.hpp"
#include "msm_host.hpp"
#include "ipa_verify_msm_host.hpp"
#include "msm_fixed_host.hpp"
#include "rp_batch_host.hpp"
#include "ipa_packed_host.hpp"
#include "ipa_wire_host.hpp"
#include "host_pool.hpp"
#include "rp_algebra_host.hpp"
#include "transcript_host.hpp"
#include "rp_wire_v2_host.hpp"
#include "rp_batch_kernels.hpp"
#include "ipa_packed_kernels.hpp"
#include "ipa_wire_kernels.hpp"
#include "rp_prove_kernels.hpp"
#include "rp_prove_mixed_kernels.hpp"
#include "ipa_prove_kernels.hpp"
#include "ipa_prove_mixed_kernels.hpp"
#include "h2c.hpp"
#include "h2c_kernels.hpp"
#include "h2c_host.hpp"

// ------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------
extern "C" {

int bpmi_version(void) { return BPMI_VERSION; }

int bpmi_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

bpmi_ctx *bpmi_ctx_create(int device, void *stream) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) { fail(nullptr, BPMI_E_NODEVICE, "no HIP device visible (libbpmi has no CPU fallback)"); return nullptr; }
  if (device < 0 || device >= n) { fail(nullptr, BPMI_E_ARG, "device index out of range"); return nullptr; }
  if (hipSetDevice(device) != hipSuccess) { fail(nullptr, BPMI_E_HIP, "hipSetDevice failed"); return nullptr; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) { fail(nullptr, BPMI_E_HIP, "hipGetDeviceProperties failed"); return nullptr; }
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    fail(nullptr, BPMI_E_NODEVICE, std::string("device is ") + prop.gcnArchName + ", libbpmi is built for gfx950 only");
    return nullptr;
  }
  bpmi_ctx *ctx = new bpmi_ctx();
  ctx->device = device;
  if (stream) { ctx->stream = (hipStream_t)stream; ctx->own_stream = false; }
  else {
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
      delete ctx; fail(nullptr, BPMI_E_HIP, "hipStreamCreate failed"); return nullptr;
    }
    ctx->own_stream = true;
  }
  return ctx;
}

void bpmi_ctx_destroy(bpmi_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)sync_lanes(ctx);
  for (auto &e : ctx->evs) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  for (auto e : ctx->ev_pool) (void)hipEventDestroy(e);
  for (Lane &l : ctx->lane) { if (l.ws) (void)hipFree(l.ws); if (l.ev_accum) (void)hipEventDestroy(l.ev_accum); if (l.ev_sorted) (void)hipEventDestroy(l.ev_sorted); }
  if (ctx->stage_in) (void)hipFree(ctx->stage_in);
  if (ctx->rp_buf) (void)hipFree(ctx->rp_buf);
  if (ctx->vflag) (void)hipHostFree(ctx->vflag);
  if (ctx->vflag_dev) (void)hipFree(ctx->vflag_dev);
  if (ctx->pin) (void)hipHostFree(ctx->pin);
  if (ctx->up_ring) (void)hipHostFree(ctx->up_ring);
  if (ctx->up_ev) (void)hipEventDestroy(ctx->up_ev);
  for (int k = 1; k < BPMI_LANES; k++) if (ctx->lane[k].stream) (void)hipStreamDestroy(ctx->lane[k].stream);
  if (ctx->stream_acc) { (void)hipStreamSynchronize(ctx->stream_acc); (void)hipStreamDestroy(ctx->stream_acc); }
  if (ctx->fold_tab) (void)hipFree(ctx->fold_tab);
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
  for (auto e : ctx->ev_slice) if (e) (void)hipEventDestroy(e);
  for (auto &pd : ctx->pend) { if (pd.pin) (void)hipHostFree(pd.pin); if (pd.done) (void)hipEventDestroy(pd.done); }
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx->helper;
  msm_graphs_clear(ctx);
  delete ctx->graphs;
  delete ctx;
}

const char *bpmi_last_error(const bpmi_ctx *ctx) {
  if (ctx) return ctx->err.c_str();
  return g_create_err.c_str();
}

int bpmi_sync(bpmi_ctx *ctx) {
  if (!ctx) return BPMI_E_ARG;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return BPMI_OK;
}

// the options and what each accepts: the table of options_host.hpp
int bpmi_set_option(bpmi_ctx *ctx, const char *name, int64_t value) {
  if (!ctx || !name) return BPMI_E_ARG;
  const OptionSet r = option_set(*ctx, name, value);
  if (r.rc) return fail(ctx, r.rc, r.msg);
  if (r.fx == OPT_FX_GRAPHS || (r.fx == OPT_FX_GRAPHS_IF_ZERO && !value)) msm_graphs_clear(ctx);
  if (r.fx == OPT_FX_FOLD_KEYS) ctx->fold_key_g = ctx->fold_key_h = nullptr;
  return BPMI_OK;
}

int bpmi_malloc(bpmi_ctx *ctx, size_t bytes, void **dptr) {
  if (!ctx || !dptr) return BPMI_E_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMalloc(dptr, bytes ? bytes : 16));
  return BPMI_OK;
}
int bpmi_free(bpmi_ctx *ctx, void *dptr) {
  if (!ctx) return BPMI_E_ARG;
  if (!dptr) return BPMI_OK;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipFree(dptr));
  return BPMI_OK;
}
int bpmi_upload(bpmi_ctx *ctx, void *dptr, const void *host, size_t bytes) {
  if (!ctx || (bytes && (!dptr || !host))) return BPMI_E_ARG;
  if (!bytes) return BPMI_OK;
  HIPCHK(ctx, h2d(ctx, dptr, host, bytes, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return BPMI_OK;
}
int bpmi_download(bpmi_ctx *ctx, void *host, const void *dptr, size_t bytes) {
  if (!ctx || (bytes && (!dptr || !host))) return BPMI_E_ARG;
  if (!bytes) return BPMI_OK;
  HIPCHK(ctx, hipMemcpyAsync(host, dptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return BPMI_OK;
}

// ---- MSM ------------------------------------------------------------------------------
static int msm_dev_impl(bpmi_ctx *ctx, const void *d_pts, const void *d_scalars, uint64_t n, uint8_t out[64]);
int bpmi_msm_dev(bpmi_ctx *ctx, const void *d_pts, const void *d_scalars, uint64_t n, uint8_t out[64]) {
  if (!ctx || !out || (n && (!d_pts || !d_scalars))) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (n > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
  if (ctx->opt_validate < 2 || n == 0) return msm_dev_impl(ctx, d_pts, d_scalars, n, out);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  PointCheck pc(ctx, "bpmi_msm_dev", ctx->stream, true);
  pc.queue(d_pts, n, "d_pts");
  int rc = pc.fetch();
  if (rc) return rc;
  rc = msm_dev_impl(ctx, d_pts, d_scalars, n, out);
  if (rc) return rc;
  rc = pc.verdict();
  if (rc) memset(out, 0, 64);
  return rc;
}
static int msm_dev_impl(bpmi_ctx *ctx, const void *d_pts, const void *d_scalars, uint64_t n, uint8_t out[64]) {
  if (!ctx || !out || (n && (!d_pts || !d_scalars))) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (n > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // (inputs of more than ~1.25 x 2^20 pairs run as slices of about 2^20 pairs, two in flight: msm_run, csrc/msm_host.hpp)
  Segs s = segs_init();
  s.pts[0] = (const u32 *)d_pts; s.sc[0] = (const u32 *)d_scalars; s.n[0] = (u32)n; s.total = (u32)n;
  return msm_run(ctx, s, out);
}
// what an MSM of n pairs runs as under the ctx's current options (no GPU work): bench.py counts its multiply-adds from this
int bpmi_msm_geometry(bpmi_ctx *ctx, uint64_t n, int pipelined, uint32_t geom[8]) {
  if (!ctx || !geom) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (n > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
  memset(geom, 0, 8 * sizeof(uint32_t));
  if (n == 0) return BPMI_OK;
  Segs s = segs_init();
  s.n[0] = (u32)n; s.total = (u32)n;
  const uint64_t K = pipelined ? 1 : msm_slice_count(*ctx, s);
  const uint64_t per = (n + K - 1) / K;
  MsmMode mode;
  mode.chained = pipelined ? ctx->opt_async_lanes != 0 : (K > 1 && per >= (1u << 19));
  const MsmPlan pl = msm_pick_geometry(*ctx, mode, per, 0, 0);
  const MsmGeom &g = pl.g;
  geom[0] = pl.small ? 1u : (pl.mid ? 2u : 0u); geom[1] = g.c; geom[2] = g.W; geom[3] = g.top2; geom[4] = g.G; geom[5] = g.L; geom[6] = (uint32_t)K; geom[7] = (uint32_t)per;
  return BPMI_OK;
}
// which accumulation the last bucket-pipeline MSM of `lane` ran (tests): waits for the lane, then reads the run table's two words
int bpmi_debug_msm_runs(bpmi_ctx *ctx, int lane, uint32_t state[3]) {
  if (!ctx || !state || lane < 0 || lane >= BPMI_LANES) return ctx ? fail(ctx, BPMI_E_ARG, "bad lane or null argument") : BPMI_E_ARG;
  memset(state, 0, 3 * sizeof(uint32_t));
  const Lane &l = ctx->lane[lane];
  if (!l.stream || !l.run_flags) return BPMI_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(l.stream));
  uint32_t words[2];
  HIPCHK(ctx, hipMemcpy(words, l.run_flags + RUN_FLAG_WORD, sizeof(words), hipMemcpyDeviceToHost));      // RUN_COUNT_WORD is the next one
  state[0] = l.run_planned; state[1] = words[0]; state[2] = words[1];
  return BPMI_OK;
}
// Asynchronous pair: enqueue returns as soon as the MSM's kernels and its device->host copy are queued on
// the ctx stream; finish waits for THAT MSM only and runs the host part of its tail.  Two slots, so the
// host tail (and the caller's own work, e.g. the exchange of partial results) of MSM k overlaps the
// kernels of MSM k + 1.
static int msm_enqueue_async(bpmi_ctx *ctx, int slot, const Segs &s, const FixedBaseCall *fx);
int bpmi_msm_dev_enqueue(bpmi_ctx *ctx, int slot, const void *d_pts, const void *d_scalars, uint64_t n) {
  if (!ctx || (n && (!d_pts || !d_scalars))) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (slot < 0 || slot >= BPMI_LANES) return fail(ctx, BPMI_E_ARG, "slot must be 0, 1 or 2");
  if (n > (1ull << 23)) return fail(ctx, BPMI_E_ARG, "bpmi_msm_dev_enqueue takes at most 2^23 pairs (use bpmi_msm_dev)");
  Segs s = segs_init();
  s.pts[0] = (const u32 *)d_pts; s.sc[0] = (const u32 *)d_scalars; s.n[0] = (u32)n; s.total = (u32)n;
  return msm_enqueue_async(ctx, slot, s, nullptr);
}
// the asynchronous enqueue behind bpmi_msm_dev_enqueue and bpmi_msm_fixed_dev_enqueue (fx: the fixed-base call, msm_fixed_host.hpp): the
// slot's state rules, the lanes of "async_lanes" and their ordering, the chained mode -- one text for both
static int msm_enqueue_async(bpmi_ctx *ctx, int slot, const Segs &s, const FixedBaseCall *fx) {
  const uint64_t n = s.total;
  if (ctx->opt_split) return fail(ctx, BPMI_E_STATE, "option split is not available with the asynchronous entry points");
  if (ctx->pend[slot].async) return fail(ctx, BPMI_E_STATE, "an MSM is still pending in this slot (bpmi_msm_finish it first)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // option async_lanes: slot 1 runs on the second lane (own stream + workspace), so the latency-bound tail stages of
  // one MSM (segmented scan, bucket reduction: few waves) overlap the throughput stages of the next one
  const int lane = ctx->opt_async_lanes ? slot : 0;
  int rc;
  if (ctx->opt_async_lanes) {
    rc = ensure_lane(ctx, 1);
    if (rc == BPMI_OK) rc = ensure_lane(ctx, 2);               // (both extra lanes exist from the first burst on: see below)
    if (rc) return rc;
  }
  if (ctx->opt_async_lanes && !ctx->async_lanes_ordered) {
    // Order EVERY extra lane after whatever produced the inputs on the ctx stream, once per burst and BEFORE this burst's first MSM
    // is queued (the option's contract: inputs complete before the first enqueue of a burst).  Recorded at a lane's first use
    // instead, the event sits behind slot 0's whole MSM: round 3 found that for lane 1 (a caller that queued a pair and waited for
    // both got them one after the other, profiles/r03_pair_modes.txt), and round 4's lane 2 still did it -- its "three in flight"
    // measurements ran on a partly serialised pipeline (re-measured: profiles/r05_pipeline_depth_ab.txt).
    HIPCHK(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->lane[1].stream, ctx->ev_fork, 0));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->lane[2].stream, ctx->ev_fork, 0));
    ctx->async_lanes_ordered = true;
  }
  MsmMode mode;
  mode.chained = ctx->opt_async_lanes != 0;
  mode.free_run = ctx->opt_accum_chain == 0;
  rc = fx ? fixed_base_enqueue(ctx, mode, lane, slot, *fx) : msm_enqueue(ctx, mode, lane, slot, s);
  if (rc == BPMI_OK) { ctx->pend[slot].async = true; ctx->pend[slot].async_empty = (n == 0); }
  return rc;
}
int bpmi_msm_finish(bpmi_ctx *ctx, int slot, uint8_t out[64]) {
  if (!ctx || !out) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (slot < 0 || slot >= BPMI_LANES) return fail(ctx, BPMI_E_ARG, "slot must be 0, 1 or 2");
  if (!ctx->pend[slot].async) return fail(ctx, BPMI_E_STATE, "no MSM was enqueued in this slot");
  ctx->pend[slot].async = false;
  if (!ctx->pend[0].async && !ctx->pend[1].async && !ctx->pend[2].async) { ctx->async_lanes_ordered = false; ctx->accum_chain_lane = -1; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // msm_finish reads an inactive slot as "n was 0" (the identity, which a verifier reads as VALID): only a slot that was enqueued
  // with n = 0 may be inactive here
  if (!ctx->pend[slot].active && !ctx->pend[slot].async_empty) return fail(ctx, BPMI_E_STATE, "the MSM of this slot was abandoned");
  return msm_finish(ctx, slot, out);
}
int bpmi_msm(bpmi_ctx *ctx, const uint8_t *pts, const uint8_t *scalars, uint64_t n, uint8_t out[64]) {
  if (!ctx || !out || (n && (!pts || !scalars))) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (n > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
  if (n == 0) { memset(out, 0, 64); return BPMI_OK; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = ensure_stage_in(ctx, 96 * n + 512);
  if (rc) return rc;
  char *dp = (char *)ctx->stage_in;
  char *ds = dp + align_up(64 * n, 256);
  HIPCHK(ctx, h2d(ctx, dp, pts, 64 * n, ctx->stream));
  HIPCHK(ctx, h2d(ctx, ds, scalars, 32 * n, ctx->stream));
  PointCheck pc(ctx, "bpmi_msm", ctx->stream, ctx->opt_validate >= 1);
  pc.queue(dp, n, "pts");
  rc = pc.fetch();
  if (rc) return rc;
  rc = msm_dev_impl(ctx, dp, ds, n, out);
  if (rc) return rc;
  rc = pc.verdict();
  if (rc) memset(out, 0, 64);
  return rc;
}

// two independent MSMs from host buffers, overlapped on the ctx's two lanes (one staging upload,
// one synchronisation): the A / S and T1 / T2 pairs of a range proof, L / R outside the IPA object
int bpmi_msm2(bpmi_ctx *ctx, const uint8_t *pts0, const uint8_t *sc0, uint64_t n0, uint8_t out0[64], const uint8_t *pts1,
              const uint8_t *sc1, uint64_t n1, uint8_t out1[64]) {
  if (!ctx || !out0 || !out1 || (n0 && (!pts0 || !sc0)) || (n1 && (!pts1 || !sc1))) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (n0 > (1ull << 23) || n1 > (1ull << 23)) return fail(ctx, BPMI_E_ARG, "bpmi_msm2 takes at most 2^23 pairs per MSM");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t o_s0 = align_up(64 * n0, 256), o_p1 = o_s0 + align_up(32 * n0, 256), o_s1 = o_p1 + align_up(64 * n1, 256);
  int rc = ensure_stage_in(ctx, o_s1 + 32 * n1 + 512);
  if (rc) return rc;
  char *d = (char *)ctx->stage_in;
  if (n0) { HIPCHK(ctx, h2d(ctx, d, pts0, 64 * n0, ctx->stream)); HIPCHK(ctx, h2d(ctx, d + o_s0, sc0, 32 * n0, ctx->stream)); }
  if (n1) { HIPCHK(ctx, h2d(ctx, d + o_p1, pts1, 64 * n1, ctx->stream)); HIPCHK(ctx, h2d(ctx, d + o_s1, sc1, 32 * n1, ctx->stream)); }
  Segs a = segs_init(), b = segs_init();
  a.pts[0] = (const u32 *)d; a.sc[0] = (const u32 *)(d + o_s0); a.n[0] = (u32)n0; a.total = (u32)n0;
  b.pts[0] = (const u32 *)(d + o_p1); b.sc[0] = (const u32 *)(d + o_s1); b.n[0] = (u32)n1; b.total = (u32)n1;
  PointCheck pc(ctx, "bpmi_msm2", ctx->stream, ctx->opt_validate >= 1);
  pc.queue(d, n0, "pts0");
  pc.queue(d + o_p1, n1, "pts1");
  rc = pc.fetch();
  if (rc) return rc;
  rc = msm_run_pair(ctx, a, out0, b, out1);
  if (rc) return rc;
  rc = pc.verdict();
  if (rc) { memset(out0, 0, 64); memset(out1, 0, 64); }
  return rc;
}

// ---- fixed-base MSM: an object that owns a point set and the table of its multiples (msm_fixed_plan_host.hpp, msm_fixed_host.hpp) ----
// the argument checks of both create calls: BPMI_E_ARG before anything is read or allocated
static int fixed_base_args(bpmi_ctx *ctx, const void *pts, uint64_t n, uint32_t window_bits, uint32_t rows, bpmi_fixed_base **out, FixedPlan &p) {
  if (!ctx) return BPMI_E_ARG;
  if (out) *out = nullptr;
  if (!pts || !out) return fail(ctx, BPMI_E_ARG, "null argument");
  p = fixed_plan(n, window_bits, rows);
  if (p.err) return fail(ctx, p.err, std::string("bpmi_fixed_base_create: ") + p.msg);
  return BPMI_OK;
}
int bpmi_fixed_base_create_dev(bpmi_ctx *ctx, const void *d_pts, uint64_t n, uint32_t window_bits, uint32_t rows, bpmi_fixed_base **out) {
  FixedPlan p;
  const int rc = fixed_base_args(ctx, d_pts, n, window_bits, rows, out, p);
  if (rc) return rc;
  return fixed_base_build(ctx, "bpmi_fixed_base_create_dev", d_pts, p, ctx->opt_validate >= 2, out);
}
int bpmi_fixed_base_create(bpmi_ctx *ctx, const uint8_t *pts, uint64_t n, uint32_t window_bits, uint32_t rows, bpmi_fixed_base **out) {
  FixedPlan p;
  int rc = fixed_base_args(ctx, pts, n, window_bits, rows, out, p);
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  rc = ensure_stage_in(ctx, 64 * n + 512);
  if (rc) return rc;
  HIPCHK(ctx, h2d(ctx, ctx->stage_in, pts, 64 * n, ctx->stream));
  return fixed_base_build(ctx, "bpmi_fixed_base_create", ctx->stage_in, p, ctx->opt_validate >= 1, out);
}
void bpmi_fixed_base_destroy(bpmi_fixed_base *fx) {
  if (!fx) return;
  (void)hipSetDevice(fx->ctx->device);
  (void)sync_lanes(fx->ctx);                     // an MSM over the table may still be queued
  if (fx->table) (void)hipFree(fx->table);
  delete fx;
}
int bpmi_fixed_base_info(const bpmi_fixed_base *fx, uint64_t info[8]) {
  if (!fx || !info) return BPMI_E_ARG;
  const FixedPlan &p = fx->plan;
  info[0] = p.n; info[1] = p.c; info[2] = p.W; info[3] = p.R; info[4] = p.Wv; info[5] = p.table_bytes; info[6] = (uint64_t)fx->build_us; info[7] = 0;
  return BPMI_OK;
}
int bpmi_fixed_base_table(bpmi_fixed_base *fx, uint32_t row, uint64_t first, uint64_t count, uint8_t *out) {
  if (!fx) return BPMI_E_ARG;
  bpmi_ctx *ctx = fx->ctx;
  if (count && !out) return fail(ctx, BPMI_E_ARG, "null argument");
  if (row >= fx->plan.R || first > fx->plan.n || count > fx->plan.n - first) return fail(ctx, BPMI_E_ARG, "bpmi_fixed_base_table: row or range outside the table");
  if (!count) return BPMI_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemcpyAsync(out, fx->table + 16ull * (fx->plan.n * row + first), 64 * count, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return BPMI_OK;
}
static int fixed_msm_args(bpmi_fixed_base *fx, const void *scalars, uint64_t n_scalars) {
  if (!fx) return BPMI_E_ARG;
  if (n_scalars && !scalars) return fail(fx->ctx, BPMI_E_ARG, "null argument");
  if (n_scalars > fx->plan.n) return fail(fx->ctx, BPMI_E_ARG, "n_scalars exceeds the object's n points");
  return BPMI_OK;
}
int bpmi_msm_fixed_dev(bpmi_fixed_base *fx, const void *d_scalars, uint64_t n_scalars, uint8_t out[64]) {
  int rc = fixed_msm_args(fx, d_scalars, n_scalars);
  if (rc) return rc;
  bpmi_ctx *ctx = fx->ctx;
  if (!out) return fail(ctx, BPMI_E_ARG, "null argument");
  if (n_scalars == 0) { memset(out, 0, 64); return BPMI_OK; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return fixed_base_run(ctx, FixedBaseCall{fx, d_scalars, n_scalars}, out);
}
int bpmi_msm_fixed(bpmi_fixed_base *fx, const uint8_t *scalars, uint64_t n_scalars, uint8_t out[64]) {
  int rc = fixed_msm_args(fx, scalars, n_scalars);
  if (rc) return rc;
  bpmi_ctx *ctx = fx->ctx;
  if (!out) return fail(ctx, BPMI_E_ARG, "null argument");
  if (n_scalars == 0) { memset(out, 0, 64); return BPMI_OK; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  rc = ensure_stage_in(ctx, 32 * n_scalars + 512);
  if (rc) return rc;
  HIPCHK(ctx, h2d(ctx, ctx->stage_in, scalars, 32 * n_scalars, ctx->stream));
  return fixed_base_run(ctx, FixedBaseCall{fx, ctx->stage_in, n_scalars}, out);
}
int bpmi_msm_fixed_dev_enqueue(bpmi_fixed_base *fx, int slot, const void *d_scalars, uint64_t n_scalars) {
  const int rc = fixed_msm_args(fx, d_scalars, n_scalars);
  if (rc) return rc;
  bpmi_ctx *ctx = fx->ctx;
  if (slot < 0 || slot >= BPMI_LANES) return fail(ctx, BPMI_E_ARG, "slot must be 0, 1 or 2");
  const FixedBaseCall call = {fx, d_scalars, n_scalars};
  Segs s = segs_init();
  s.total = (u32)n_scalars;                      // (what the slot's bookkeeping reads: an MSM of no scalars leaves it empty)
  return msm_enqueue_async(ctx, slot, s, &call);
}

// ---- batched point ops --------------------------------------------------------------------
int bpmi_ec_mul_batch_dev(bpmi_ctx *ctx, const void *d_pts, const void *d_scalars, uint64_t n, void *d_out) {
  if (!ctx || (n && (!d_pts || !d_scalars || !d_out))) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (n > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
  if (n == 0) return BPMI_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (n < (uint64_t)MULB_MIN_N || ctx->opt_mulb == 0) {            // few points: the table kernel's inversion chain is not worth its latency
    StageTimer t(ctx, ST_MULBATCH);
    hipLaunchKernelGGL(k_ec_mul_batch, dim3((u32)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const u32 *)d_pts,
                       (const u32 *)d_scalars, (u32)n, (u32 *)d_out);
    HIPCHK(ctx, hipGetLastError());
    return BPMI_OK;
  }
  // slices of 3 x 65 536 points: three waves on every SIMD (the kernels' occupancy) in ONE round, and a bounded workspace
  // (affine 3P, 5P, 7P: 216 B per point; the table kernel's scratch columns: 864 B per point as it is laid out for two arrays)
  const uint64_t slice = 3ull << 16;
  const uint64_t m0 = std::min<uint64_t>(n, slice), nthr0 = (m0 + ODDMUL_PER_THREAD_MULB - 1) / ODDMUL_PER_THREAD_MULB;
  const size_t tab_bytes = align_up(3 * 72 * (size_t)m0, 256), scr_bytes = 144 * 3 * (size_t)ODDMUL_PER_THREAD_MULB * 2 * nthr0;
  int rc = ensure_ws(ctx, tab_bytes + scr_bytes);
  if (rc) return rc;
  u32 *tab = (u32 *)ctx->lane[0].ws, *scr = (u32 *)((char *)ctx->lane[0].ws + tab_bytes);
  for (uint64_t base = 0; base < n; base += slice) {
    const u32 m = (u32)std::min<uint64_t>(slice, n - base), nthr = (m + ODDMUL_PER_THREAD_MULB - 1) / ODDMUL_PER_THREAD_MULB;
    const u32 *p = (const u32 *)d_pts + 16 * base, *k = (const u32 *)d_scalars + 8 * base;
    StageTimer t(ctx, ST_MULBATCH);
    hipLaunchKernelGGL(k_ec_odd_multiples<ODDMUL_PER_THREAD_MULB>, dim3((nthr + 255) / 256), dim3(256), 0, ctx->stream, p, (const u32 *)nullptr, m, tab,
                       (u32 *)nullptr, scr);
    hipLaunchKernelGGL(k_ec_mul_batch_glv, dim3((m + 255) / 256), dim3(256), 0, ctx->stream, p, k, m, (const u32 *)tab, (u32 *)d_out + 16 * base);
  }
  HIPCHK(ctx, hipGetLastError());
  return BPMI_OK;
}
int bpmi_ec_mul_batch(bpmi_ctx *ctx, const uint8_t *pts, const uint8_t *scalars, uint64_t n, uint8_t *out) {
  if (!ctx || (n && (!pts || !scalars || !out))) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (n > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
  if (n == 0) return BPMI_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = ensure_stage_in(ctx, 160 * n + 1024);
  if (rc) return rc;
  char *dp = (char *)ctx->stage_in, *ds = dp + align_up(64 * n, 256), *dout = ds + align_up(32 * n, 256);
  HIPCHK(ctx, h2d(ctx, dp, pts, 64 * n, ctx->stream));
  HIPCHK(ctx, h2d(ctx, ds, scalars, 32 * n, ctx->stream));
  PointCheck pc(ctx, "bpmi_ec_mul_batch", ctx->stream, ctx->opt_validate >= 1);
  pc.queue(dp, n, "pts");
  rc = pc.fetch();
  if (rc) return rc;
  rc = bpmi_ec_mul_batch_dev(ctx, dp, ds, n, dout);
  if (rc) return rc;
  if (pc.on) {                                   // the verdict before anything is written to the caller's buffer
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    rc = pc.verdict();
    if (rc) return rc;
  }
  HIPCHK(ctx, hipMemcpyAsync(out, dout, 64 * n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return BPMI_OK;
}
static void make_naf_pair(NafPair &nf, const uint8_t k1[32], const uint8_t k2[32]) {
  nf.top = -1;
  host_naf(k1, nf.nz1, nf.sg1, nf.top);
  host_naf(k2, nf.nz2, nf.sg2, nf.top);
}
// out_a[i] = ka1 * a1[i] + ka2 * a2[i] (i < na)  and  out_b[i] = kb1 * b1[i] + kb2 * b2[i] (i < nb), one launch
static int lincomb2_pair_dev(bpmi_ctx *ctx, const void *a1, const void *a2, const uint8_t ka1[32], const uint8_t ka2[32], uint64_t na, void *out_a,
                             const void *b1, const void *b2, const uint8_t kb1[32], const uint8_t kb2[32], uint64_t nb, void *out_b) {
  LincombJob ja = {(const u32 *)a1, (const u32 *)a2, (u32 *)out_a, (u32)na};
  LincombJob jb = {(const u32 *)b1, (const u32 *)b2, (u32 *)out_b, (u32)nb};
  NafPair nfa, nfb;
  make_naf_pair(nfa, ka1, ka2);
  if (nb) make_naf_pair(nfb, kb1, kb2); else { memset(&nfb, 0, sizeof(nfb)); nfb.top = -1; }
  const uint64_t total = na + nb;
  {
    StageTimer t(ctx, ST_LINCOMB2);
    hipLaunchKernelGGL(k_ec_lincomb2, dim3((u32)((total + 255) / 256)), dim3(256), 0, ctx->stream, ja, nfa, jb, nfb);
  }
  HIPCHK(ctx, hipGetLastError());
  return BPMI_OK;
}
int bpmi_ec_lincomb2_batch_dev(bpmi_ctx *ctx, const void *d_p1, const void *d_p2, const uint8_t k1[32], const uint8_t k2[32],
                               uint64_t n, void *d_out) {
  if (!ctx || !k1 || !k2 || (n && (!d_p1 || !d_p2 || !d_out))) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (n > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
  if (n == 0) return BPMI_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return lincomb2_pair_dev(ctx, d_p1, d_p2, k1, k2, n, d_out, nullptr, nullptr, nullptr, nullptr, 0, nullptr);
}
int bpmi_ec_lincomb2_batch(bpmi_ctx *ctx, const uint8_t *p1, const uint8_t *p2, const uint8_t k1[32], const uint8_t k2[32],
                           uint64_t n, uint8_t *out) {
  if (!ctx || !k1 || !k2 || (n && (!p1 || !p2 || !out))) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (n > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
  if (n == 0) return BPMI_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = ensure_stage_in(ctx, 192 * n + 1024);
  if (rc) return rc;
  char *d1 = (char *)ctx->stage_in, *d2 = d1 + align_up(64 * n, 256), *dout = d2 + align_up(64 * n, 256);
  HIPCHK(ctx, h2d(ctx, d1, p1, 64 * n, ctx->stream));
  HIPCHK(ctx, h2d(ctx, d2, p2, 64 * n, ctx->stream));
  PointCheck pc(ctx, "bpmi_ec_lincomb2_batch", ctx->stream, ctx->opt_validate >= 1);
  pc.queue(d1, n, "p1");
  pc.queue(d2, n, "p2");
  rc = pc.fetch();
  if (rc) return rc;
  rc = bpmi_ec_lincomb2_batch_dev(ctx, d1, d2, k1, k2, n, dout);
  if (rc) return rc;
  if (pc.on) {
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    rc = pc.verdict();
    if (rc) return rc;
  }
  HIPCHK(ctx, hipMemcpyAsync(out, dout, 64 * n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return BPMI_OK;
}
int bpmi_ec_sum(bpmi_ctx *ctx, const uint8_t *pts, uint64_t n, uint8_t out[64]) {
  if (!ctx || !out || (n && !pts)) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (n > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
  if (n == 0) { memset(out, 0, 64); return BPMI_OK; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = ensure_stage_in(ctx, 64 * n + 512);
  if (rc) return rc;
  char *dp = (char *)ctx->stage_in, *dout = dp + align_up(64 * n, 256);
  HIPCHK(ctx, h2d(ctx, dp, pts, 64 * n, ctx->stream));
  // (the per-GPU partial results a sharded caller folds here are the library's own outputs; a few points: checked on the host)
  PointCheck pc(ctx, "bpmi_ec_sum", ctx->stream, ctx->opt_validate >= 1);
  if (n <= VALIDATE_HOST_MAX) { rc = pc.host(pts, n, "pts"); if (rc) { memset(out, 0, 64); return rc; } }
  else pc.queue(dp, n, "pts");
  rc = pc.fetch();
  if (rc) return rc;
  {
    StageTimer t(ctx, ST_MISC);
    hipLaunchKernelGGL(k_ec_sum, dim3(1), dim3(256), 0, ctx->stream, (const u32 *)dp, (u32)n, (u32 *)dout);
  }
  uint8_t tmp[64];
  HIPCHK(ctx, hipMemcpyAsync(tmp, dout, 64, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  rc = pc.verdict();
  if (rc) { memset(out, 0, 64); return rc; }               // as bpmi_msm: a refused call leaves the identity's bytes, never a stale value
  memcpy(out, tmp, 64);
  return BPMI_OK;
}

int bpmi_ec_sum_dev(bpmi_ctx *ctx, const void *d_pts, uint64_t n, uint8_t out[64]) {
  if (!ctx || !out || (n && !d_pts)) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (n > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
  if (n == 0) { memset(out, 0, 64); return BPMI_OK; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = ensure_stage_in(ctx, 512);
  if (rc) return rc;
  {
    StageTimer t(ctx, ST_MISC);
    hipLaunchKernelGGL(k_ec_sum, dim3(1), dim3(256), 0, ctx->stream, (const u32 *)d_pts, (u32)n, (u32 *)ctx->stage_in);
  }
  HIPCHK(ctx, hipMemcpyAsync(out, ctx->stage_in, 64, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return BPMI_OK;
}

// the fold without the wait: the canonical affine sum is written to d_out (64 B of device memory) by a kernel queued on the ctx
// stream; the caller reads it after bpmi_sync / bpmi_download (a pipelined caller overlaps the fold of step j with step j + 1)
int bpmi_ec_sum_dev_enqueue(bpmi_ctx *ctx, const void *d_pts, uint64_t n, void *d_out) {
  if (!ctx || !d_out || (n && !d_pts)) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (n > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (n == 0) { HIPCHK(ctx, hipMemsetAsync(d_out, 0, 64, ctx->stream)); return BPMI_OK; }
  {
    StageTimer t(ctx, ST_MISC);
    hipLaunchKernelGGL(k_ec_sum, dim3(1), dim3(256), 0, ctx->stream, (const u32 *)d_pts, (u32)n, (u32 *)d_out);
  }
  HIPCHK(ctx, hipGetLastError());
  return BPMI_OK;
}

int bpmi_ec_decompress_batch(bpmi_ctx *ctx, const uint8_t *comp, uint64_t n, uint8_t *out, uint8_t *ok) {
  if (!ctx || (n && (!comp || !out || !ok))) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (n > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
  if (n == 0) return BPMI_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = ensure_stage_in(ctx, 98 * n + 1024);
  if (rc) return rc;
  char *din = (char *)ctx->stage_in, *dout = din + align_up(33 * n, 256), *dok = dout + align_up(64 * n, 256);
  HIPCHK(ctx, h2d(ctx, din, comp, 33 * n, ctx->stream));
  {
    StageTimer t(ctx, ST_DECOMP);
    hipLaunchKernelGGL(k_ec_decompress, dim3((u32)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const uint8_t *)din, (u32)n,
                       (u32 *)dout, (uint8_t *)dok);
  }
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(out, dout, 64 * n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ok, dok, n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return BPMI_OK;
}

// the same with the points left in device memory (d_out: n x 64 B on the ctx's device), e.g. straight into the point array of
// the batch verifier's one MSM: no copy of the decompressed points to the host and back
int bpmi_ec_decompress_batch_dev(bpmi_ctx *ctx, const uint8_t *comp, uint64_t n, void *d_out, uint8_t *ok) {
  if (!ctx || (n && (!comp || !d_out || !ok))) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (n > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
  if (n == 0) return BPMI_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = ensure_stage_in(ctx, 34 * n + 1024);
  if (rc) return rc;
  char *din = (char *)ctx->stage_in, *dok = din + align_up(33 * n, 256);
  HIPCHK(ctx, h2d(ctx, din, comp, 33 * n, ctx->stream));
  {
    StageTimer t(ctx, ST_DECOMP);
    hipLaunchKernelGGL(k_ec_decompress, dim3((u32)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const uint8_t *)din, (u32)n, (u32 *)d_out, (uint8_t *)dok);
  }
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(ok, dok, n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return BPMI_OK;
}
// ---- bulk hash to the curve (h2c_host.hpp) --------------------------------------------------------------------------------------------
int bpmi_ec_hash_batch(bpmi_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off, uint64_t n, uint32_t max_tries, uint8_t *out, uint8_t *tries) {
  if (!ctx) return BPMI_E_ARG;
  uint64_t total = 0;
  const int rc = h2c_check(ctx, false, msgs, msg_off, 0, 0, 0, n, max_tries, out, &total);
  return rc ? rc : h2c_run(ctx, false, msgs, total, msg_off, 0, n, max_tries, nullptr, out, tries);
}
int bpmi_ec_hash_batch_dev(bpmi_ctx *ctx, const uint8_t *msgs, const uint64_t *msg_off, uint64_t n, uint32_t max_tries, void *d_out, uint8_t *tries) {
  if (!ctx) return BPMI_E_ARG;
  uint64_t total = 0;
  const int rc = h2c_check(ctx, false, msgs, msg_off, 0, 0, 0, n, max_tries, d_out, &total);
  return rc ? rc : h2c_run(ctx, false, msgs, total, msg_off, 0, n, max_tries, d_out, nullptr, tries);
}
int bpmi_ec_hash_range(bpmi_ctx *ctx, const uint8_t *tail, uint64_t tail_len, uint64_t lo, uint64_t hi, uint32_t max_tries, uint8_t *out, uint8_t *tries) {
  if (!ctx) return BPMI_E_ARG;
  uint64_t total = 0;
  const int rc = h2c_check(ctx, true, tail, nullptr, tail_len, lo, hi, 0, max_tries, out, &total);
  return rc ? rc : h2c_run(ctx, true, tail, total, nullptr, lo, hi - lo, max_tries, nullptr, out, tries);
}
int bpmi_ec_hash_range_dev(bpmi_ctx *ctx, const uint8_t *tail, uint64_t tail_len, uint64_t lo, uint64_t hi, uint32_t max_tries, void *d_out, uint8_t *tries) {
  if (!ctx) return BPMI_E_ARG;
  uint64_t total = 0;
  const int rc = h2c_check(ctx, true, tail, nullptr, tail_len, lo, hi, 0, max_tries, d_out, &total);
  return rc ? rc : h2c_run(ctx, true, tail, total, nullptr, lo, hi - lo, max_tries, d_out, nullptr, tries);
}
int bpmi_memcpy_dev(bpmi_ctx *ctx, void *d_dst, const void *d_src, size_t bytes) {
  if (!ctx || (bytes && (!d_dst || !d_src))) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (!bytes) return BPMI_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  return BPMI_OK;
}
// one MSM over up to three (points, scalars) arrays that live in different device buffers -- no gather / concat
int bpmi_msm_segs_dev(bpmi_ctx *ctx, uint32_t nseg, const void *const *d_pts, const void *const *d_scalars, const uint64_t *n, uint8_t out[64]) {
  if (!ctx || !out || (nseg && (!d_pts || !d_scalars || !n))) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (nseg > 3) return fail(ctx, BPMI_E_ARG, "at most three segments");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Segs s = segs_init();
  uint64_t total = 0;
  u32 k = 0;
  for (u32 i = 0; i < nseg; i++) {
    if (!n[i]) continue;
    if (!d_pts[i] || !d_scalars[i]) return fail(ctx, BPMI_E_ARG, "null segment");
    s.pts[k] = (const u32 *)d_pts[i]; s.sc[k] = (const u32 *)d_scalars[i]; s.n[k] = (u32)n[i];
    total += n[i];
    k++;
  }
  if (total > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
  s.total = (u32)total;
  return msm_run(ctx, s, out);
}

// ---- scalar ops -------------------------------------------------------------------------------
// njobs (1 or 2) inner products of length n in two launches; d_partial: njobs x SC_DOT_MAX_BLOCKS x 32 B
static int sc_dot_jobs(bpmi_ctx *ctx, const DotJobs &jobs, u32 njobs, uint64_t n, u32 *d_partial) {
  const u32 nb = n <= 4096 ? 1u : (u32)std::min<uint64_t>((n + 255) / 256, SC_DOT_MAX_BLOCKS);
  StageTimer t(ctx, ST_SCDOT);
  hipLaunchKernelGGL(k_sc_dot, dim3(nb, njobs), dim3(256), 0, ctx->stream, jobs, (u32)n, d_partial);
  if (nb > 1) hipLaunchKernelGGL(k_sc_sum, dim3(njobs), dim3(256), 0, ctx->stream, (const u32 *)d_partial, nb, jobs);
  return BPMI_OK;
}
static int sc_dot_dev_to(bpmi_ctx *ctx, const void *d_a, const void *d_b, uint64_t n, u32 *d_out, u32 *d_partial) {
  DotJobs j;
  j.a[0] = j.a[1] = (const u32 *)d_a; j.b[0] = j.b[1] = (const u32 *)d_b; j.out[0] = j.out[1] = d_out;
  return sc_dot_jobs(ctx, j, 1, n, d_partial);
}
int bpmi_sc_dot_dev(bpmi_ctx *ctx, const void *d_a, const void *d_b, uint64_t n, uint8_t out[32]) {
  if (!ctx || !out || (n && (!d_a || !d_b))) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (n > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
  if (n == 0) { memset(out, 0, 32); return BPMI_OK; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = ensure_ws(ctx, 32 * 1024 + 256);
  if (rc) return rc;
  u32 *partial = (u32 *)ctx->lane[0].ws, *dout = partial + 8 * 1024;
  sc_dot_dev_to(ctx, d_a, d_b, n, dout, partial);
  rc = ensure_pin(ctx, 4096);
  if (rc) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->pin, dout, 32, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(out, ctx->pin, 32);
  return BPMI_OK;
}
int bpmi_sc_dot(bpmi_ctx *ctx, const uint8_t *a, const uint8_t *b, uint64_t n, uint8_t out[32]) {
  if (!ctx || !out || (n && (!a || !b))) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (n > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
  if (n == 0) { memset(out, 0, 32); return BPMI_OK; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = ensure_stage_in(ctx, 64 * n + 512);
  if (rc) return rc;
  char *da = (char *)ctx->stage_in, *db = da + align_up(32 * n, 256);
  HIPCHK(ctx, h2d(ctx, da, a, 32 * n, ctx->stream));
  HIPCHK(ctx, h2d(ctx, db, b, 32 * n, ctx->stream));
  return bpmi_sc_dot_dev(ctx, da, db, n, out);
}
int bpmi_sc_fold_dev(bpmi_ctx *ctx, const void *d_lo, const void *d_hi, const uint8_t x[32], const uint8_t y[32], uint64_t n, void *d_out) {
  if (!ctx || !x || !y || (n && (!d_lo || !d_hi || !d_out))) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (n > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
  if (n == 0) return BPMI_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  FoldJobs fj;
  fj.lo[0] = fj.lo[1] = (const u32 *)d_lo; fj.hi[0] = fj.hi[1] = (const u32 *)d_hi; fj.out[0] = fj.out[1] = (u32 *)d_out;
  memcpy(fj.xy[0].k1, x, 32); memcpy(fj.xy[0].k2, y, 32);
  fj.xy[1] = fj.xy[0];
  {
    StageTimer t(ctx, ST_SCFOLD);
    hipLaunchKernelGGL(k_sc_fold, dim3((u32)((n + 255) / 256), 1), dim3(256), 0, ctx->stream, fj, (u32)n);
  }
  HIPCHK(ctx, hipGetLastError());
  return BPMI_OK;
}
int bpmi_sc_fold(bpmi_ctx *ctx, const uint8_t *lo, const uint8_t *hi, const uint8_t x[32], const uint8_t y[32], uint64_t n, uint8_t *out) {
  if (!ctx || !x || !y || (n && (!lo || !hi || !out))) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (n > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
  if (n == 0) return BPMI_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = ensure_stage_in(ctx, 96 * n + 1024);
  if (rc) return rc;
  char *dl = (char *)ctx->stage_in, *dh = dl + align_up(32 * n, 256), *dout = dh + align_up(32 * n, 256);
  HIPCHK(ctx, h2d(ctx, dl, lo, 32 * n, ctx->stream));
  HIPCHK(ctx, h2d(ctx, dh, hi, 32 * n, ctx->stream));
  rc = bpmi_sc_fold_dev(ctx, dl, dh, x, y, n, dout);
  if (rc) return rc;
  HIPCHK(ctx, hipMemcpyAsync(out, dout, 32 * n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return BPMI_OK;
}

// ---- IPA verifier: s-vector on the device + ONE multi-segment MSM ---------------------------------------------
// layout in ctx->stage_in: sa (32 n) | sb (32 n) | x table (64 k) | half tables | extra area
struct SvecLayout { u32 *sa, *sb, *xt, *tab; char *extra; u32 k, kl; };
static int svector_layout(bpmi_ctx *ctx, uint64_t n, u32 k, size_t extra_bytes, SvecLayout &L) {
  const u32 kl = k / 2, kh = k - kl;
  const size_t ntab = ((size_t)1 << kl) + ((size_t)1 << kh);
  const size_t o_sb = align_up(32 * n, 256), o_xt = o_sb + align_up(32 * n, 256), o_tab = o_xt + align_up(64 * (size_t)(k ? k : 1), 256),
               o_ex = o_tab + align_up(64 * ntab, 256);
  int rc = ensure_stage_in(ctx, o_ex + extra_bytes + 512);
  if (rc) return rc;
  char *base = (char *)ctx->stage_in;
  L.sa = (u32 *)base; L.sb = (u32 *)(base + o_sb); L.xt = (u32 *)(base + o_xt); L.tab = (u32 *)(base + o_tab); L.extra = base + o_ex;
  L.k = k; L.kl = kl;
  return BPMI_OK;
}
static int svector_launch(bpmi_ctx *ctx, const SvecLayout &L, const void *d_scale, uint64_t n, const uint8_t *xs, const uint8_t *xinvs,
                          const uint8_t a[32], const uint8_t b[32]) {
  const u32 k = L.k;
  const size_t ntab = ((size_t)1 << L.kl) + ((size_t)1 << (k - L.kl));
  std::vector<uint8_t> xt(64 * (size_t)(k ? k : 1));
  for (u32 j = 0; j < k; j++) { memcpy(&xt[64 * j], xs + 32 * j, 32); memcpy(&xt[64 * j + 32], xinvs + 32 * j, 32); }
  HIPCHK(ctx, h2d(ctx, L.xt, xt.data(), xt.size(), ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));          // xt is owned by this frame
  Sc2 ab;
  memcpy(ab.k1, a, 32); memcpy(ab.k2, b, 32);
  {
    StageTimer t(ctx, ST_SCFOLD);
    hipLaunchKernelGGL(k_sc_svector_tables, dim3((u32)((ntab + 255) / 256)), dim3(256), 0, ctx->stream, L.xt, k, L.kl, ab, L.tab);
    hipLaunchKernelGGL(k_sc_svector, dim3((u32)((n + 255) / 256)), dim3(256), 0, ctx->stream, L.tab, k, L.kl, (const u32 *)d_scale, (u32)n, L.sa, L.sb);
  }
  HIPCHK(ctx, hipGetLastError());
  return BPMI_OK;
}

int bpmi_sc_svector(bpmi_ctx *ctx, const uint8_t *xs, const uint8_t *xinvs, uint32_t k, const uint8_t a[32], const uint8_t b[32],
                    const uint8_t *scale, uint8_t *sa, uint8_t *sb) {
  if (!ctx || !a || !b || !sa || !sb || (k && (!xs || !xinvs))) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (k > 24) return fail(ctx, BPMI_E_ARG, "k must be <= 24");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const uint64_t n = 1ull << k;
  SvecLayout L;
  int rc = svector_layout(ctx, n, k, scale ? 32 * n : 0, L);
  if (rc) return rc;
  if (scale) HIPCHK(ctx, h2d(ctx, L.extra, scale, 32 * n, ctx->stream));
  rc = svector_launch(ctx, L, scale ? L.extra : nullptr, n, xs, xinvs, a, b);
  if (rc) return rc;
  HIPCHK(ctx, hipMemcpyAsync(sa, L.sa, 32 * n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(sb, L.sb, 32 * n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return BPMI_OK;
}

int bpmi_ipa_verify_dev(bpmi_ctx *ctx, const void *d_g, const void *d_h, const void *d_hscale, uint64_t n, const uint8_t *xs, const uint8_t *xinvs,
                        uint32_t k, const uint8_t a[32], const uint8_t b[32], const uint8_t *extra_pts, const uint8_t *extra_scalars,
                        uint64_t n_extra, uint8_t out[64]) {
  if (!ctx || !d_g || !d_h || !a || !b || !out || (k && (!xs || !xinvs)) || (n_extra && (!extra_pts || !extra_scalars)))
    return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  u32 kk;
  if (!log2_exact(n, kk) || kk != k || n > (1ull << 22)) return fail(ctx, BPMI_E_ARG, "n must be 2^k, k <= 22");
  if (n_extra > (1u << 20)) return fail(ctx, BPMI_E_ARG, "too many extra points");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t o_es = align_up(64 * n_extra, 256);
  SvecLayout L;
  int rc = svector_layout(ctx, n, k, o_es + 32 * n_extra, L);
  if (rc) return rc;
  // a few extra points are checked on the host, many by the kernel; the generators from level 2
  PointCheck pc(ctx, "bpmi_ipa_verify_dev", ctx->stream, ctx->opt_validate >= 1);
  const bool extra_on_host = n_extra <= VALIDATE_HOST_MAX;
  if (extra_on_host) { rc = pc.host(extra_pts, n_extra, "extra_pts"); if (rc) return rc; }
  rc = svector_launch(ctx, L, d_hscale, n, xs, xinvs, a, b);
  if (rc) return rc;
  char *d_ex = L.extra;
  if (n_extra) {
    HIPCHK(ctx, h2d(ctx, d_ex, extra_pts, 64 * n_extra, ctx->stream));
    HIPCHK(ctx, h2d(ctx, d_ex + o_es, extra_scalars, 32 * n_extra, ctx->stream));
  }
  return ipa_verify_msm(ctx, pc, d_g, d_h, n, L.sa, L.sb, d_ex, d_ex + o_es, n_extra, !extra_on_host, false, out);
}

}  // extern "C"

#include "ipa_host.hpp"
#include "ipa_batch_host.hpp"
#include "ipa_mixed_host.hpp"
#include "ipa_packed_dev_host.hpp"
#include "ipa_packed_mixed_dev_host.hpp"
#include "ipa_wire_dev_host.hpp"
#include "ipa_group_dev_host.hpp"
#include "ipa_group_mixed_dev_host.hpp"
#include "msm_batch_host.hpp"
#include "rp_batch_dev_host.hpp"
#include "rp_mixed_dev_host.hpp"
#include "rp_group_mixed_dev_host.hpp"

extern "C" {

// page-locked host memory for buffers that are handed to the library again and again (e.g. the receive buffer of wire proofs:
// uploads from it run at link speed and without a staging copy)
int bpmi_host_alloc(bpmi_ctx *ctx, size_t bytes, void **out) {
  if (!ctx || !out || !bytes) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipHostMalloc(out, bytes, hipHostMallocDefault));
  return BPMI_OK;
}
int bpmi_host_free(bpmi_ctx *ctx, void *p) {
  if (!ctx) return BPMI_E_ARG;
  if (!p) return BPMI_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipHostFree(p));
  return BPMI_OK;
}

// ---- self-test hook ----------------------------------------------------------------------------------------------
int bpmi_debug_fe_op(bpmi_ctx *ctx, int op, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint64_t n, uint32_t *out) {
  if (!ctx || !a || !b || !c || !d || !out) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (n == 0) return BPMI_OK;
  if (n > (1u << 22)) return fail(ctx, BPMI_E_ARG, "n too large");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t bytes = 36 * n, stride = align_up(bytes, 256);
  int rc = ensure_stage_in(ctx, 5 * stride + 512);
  if (rc) return rc;
  char *base = (char *)ctx->stage_in;
  const uint32_t *src[4] = {a, b, c, d};
  for (int k = 0; k < 4; k++) HIPCHK(ctx, h2d(ctx, base + k * stride, src[k], bytes, ctx->stream));
  hipLaunchKernelGGL(k_debug_fe_op, dim3((u32)((n + 255) / 256)), dim3(256), 0, ctx->stream, op, (const u32 *)base, (const u32 *)(base + stride),
                     (const u32 *)(base + 2 * stride), (const u32 *)(base + 3 * stride), (u32)n, (u32 *)(base + 4 * stride));
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(out, base + 4 * stride, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return BPMI_OK;
}

// the four-lane point addition of the bucket reduction (quad_add, msm_kernels.hpp) on n pairs of 144-byte XYZZ records
int bpmi_debug_quad_add(bpmi_ctx *ctx, const uint32_t *a, const uint32_t *b, uint64_t n, uint32_t *out) {
  if (!ctx || !a || !b || !out) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (n == 0) return BPMI_OK;
  if (n > (1u << 20)) return fail(ctx, BPMI_E_ARG, "n too large");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t bytes = 4 * XYZZ_WORDS * n, stride = align_up(bytes, 256);
  int rc = ensure_stage_in(ctx, 3 * stride + 512);
  if (rc) return rc;
  char *base = (char *)ctx->stage_in;
  HIPCHK(ctx, h2d(ctx, base, a, bytes, ctx->stream));
  HIPCHK(ctx, h2d(ctx, base + stride, b, bytes, ctx->stream));
  hipLaunchKernelGGL(k_debug_quad_add, dim3((u32)((4 * n + 255) / 256)), dim3(256), 0, ctx->stream, (const u32 *)base, (const u32 *)(base + stride), (u32)n,
                     (u32 *)(base + 2 * stride));
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(out, base + 2 * stride, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return BPMI_OK;
}

// the group law of curve.hpp (k_debug_point_op, point_kernels.hpp) on n raw 144-byte records; ops: include/bpmi.h
int bpmi_debug_point_op(bpmi_ctx *ctx, int op, const uint32_t *a, const uint32_t *b, uint64_t n, uint32_t *out) {
  if (!ctx || !a || !b || !out) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (op < 0 || op > 9) return fail(ctx, BPMI_E_ARG, "unknown op");
  if (n == 0) return BPMI_OK;
  if (n > (1u << 20)) return fail(ctx, BPMI_E_ARG, "n too large");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t bytes = 4 * XYZZ_WORDS * n, stride = align_up(bytes, 256);
  int rc = ensure_stage_in(ctx, 3 * stride + 512);
  if (rc) return rc;
  char *base = (char *)ctx->stage_in;
  HIPCHK(ctx, h2d(ctx, base, a, bytes, ctx->stream));
  HIPCHK(ctx, h2d(ctx, base + stride, b, bytes, ctx->stream));
  hipLaunchKernelGGL(k_debug_point_op, dim3((u32)((n + 255) / 256)), dim3(256), 0, ctx->stream, op, (const u32 *)base, (const u32 *)(base + stride), (u32)n,
                     (u32 *)(base + 2 * stride));
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(out, base + 2 * stride, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return BPMI_OK;
}

// ---- profiling -----------------------------------------------------------------------------------
static void prof_drain(bpmi_ctx *ctx) {
  (void)hipStreamSynchronize(ctx->stream);
  for (auto &e : ctx->evs) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) { ctx->prof_ms[e.stage] += ms; ctx->prof_calls[e.stage]++; }
    ctx->ev_pool.push_back(e.a); ctx->ev_pool.push_back(e.b);
  }
  ctx->evs.clear();
}
int bpmi_profile(bpmi_ctx *ctx, int enable) {
  if (!ctx) return BPMI_E_ARG;
  prof_drain(ctx);
  ctx->prof = enable != 0;
  ctx->prof_only = enable == 2 ? ST_ACCUM : -1;
  return BPMI_OK;
}
int bpmi_profile_reset(bpmi_ctx *ctx) {
  if (!ctx) return BPMI_E_ARG;
  prof_drain(ctx);
  for (int i = 0; i < BPMI_NSTAGES; i++) { ctx->prof_ms[i] = 0; ctx->prof_calls[i] = 0; }
  return BPMI_OK;
}
int bpmi_profile_read(bpmi_ctx *ctx, double ms[BPMI_NSTAGES], uint64_t calls[BPMI_NSTAGES]) {
  if (!ctx || !ms || !calls) return BPMI_E_ARG;
  prof_drain(ctx);
  for (int i = 0; i < BPMI_NSTAGES; i++) { ms[i] = ctx->prof_ms[i]; calls[i] = ctx->prof_calls[i]; }
  return BPMI_OK;
}
const char *bpmi_profile_stage_name(int stage) {
  if (stage < 0 || stage >= BPMI_NSTAGES) return "";
  return STAGE_NAMES[stage];
}

}  // extern "C"

#include "prove_shared_host.hpp"
#include "rp_prove_host.hpp"
#include "rp_prove_mixed_host.hpp"
#include "ipa_prove_host.hpp"
