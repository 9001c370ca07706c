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
// This file: the C-ABI entry points.  The inner-product prover (the IPA state object, deferred generator folding) is ipa_host.hpp,
// included below where its section stood.
// Kernels and host orchestration live in the *.hpp files included below (one translation unit).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
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
#include "msm_plan_host.hpp"
#include "context.hpp"
#include "device_util.hpp"
#include "msm_kernels.hpp"
#include "fold_ops_host.hpp"
#include "point_kernels.hpp"
#include "scalar_kernels.hpp"
#include "host_tail.hpp"
#include "msm_host.hpp"
#include "rp_batch_host.hpp"
#include "host_pool.hpp"
#include "rp_algebra_host.hpp"
#include "transcript_host.hpp"
#include "rp_wire_v2_host.hpp"
#include "rp_batch_kernels.hpp"
#include "rp_prove_kernels.hpp"

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

int bpmi_set_option(bpmi_ctx *ctx, const char *name, int64_t value) {
  if (!ctx || !name) return BPMI_E_ARG;
  if (!strcmp(name, "window_bits")) { if (value != 0 && (value < 2 || value > 16)) return fail(ctx, BPMI_E_ARG, "window_bits must be 0 or 2..16"); ctx->opt_c = (int)value; return BPMI_OK; }
  if (!strcmp(name, "accum_stream")) { if (value < 0 || value > 2) return fail(ctx, BPMI_E_ARG, "accum_stream must be 0, 1 or 2"); ctx->opt_accum_stream = (int)value; return BPMI_OK; }
  if (!strcmp(name, "lane_priority")) { if (value < -1 || value > 1) return fail(ctx, BPMI_E_ARG, "lane_priority must be -1, 0 or 1"); ctx->opt_lane_prio = (int)value; return BPMI_OK; }
  if (!strcmp(name, "pair_sched")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "pair_sched must be 0 or 1"); ctx->opt_pair_sched = (int)value; return BPMI_OK; }
  if (!strcmp(name, "prover_wire_format")) { if (value != 2 && value != 3) return fail(ctx, BPMI_E_ARG, "prover_wire_format must be 2 or 3"); ctx->opt_prover_wire = (int)value; return BPMI_OK; }
  if (!strcmp(name, "prover_split")) { if (value < 0 || value > (1 << 20)) return fail(ctx, BPMI_E_ARG, "prover_split must be 0, 1 or the smallest half"); ctx->opt_prover_split = (int)value; return BPMI_OK; }
  if (!strcmp(name, "rounds")) { if (value < 0 || value > 16) return fail(ctx, BPMI_E_ARG, "rounds must be 0 .. 16"); ctx->opt_rounds = (int)value; msm_graphs_clear(ctx); return BPMI_OK; }
  if (!strcmp(name, "pair_rounds")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "pair_rounds must be 0 or 1"); ctx->opt_pair_rounds = (int)value; return BPMI_OK; }
  if (!strcmp(name, "accum_chain")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "accum_chain must be 0 or 1"); ctx->opt_accum_chain = (int)value; return BPMI_OK; }
  if (!strcmp(name, "slice_n")) { if (value < -1 || value > (1 << 23) || (value > 0 && value < (1 << 16))) return fail(ctx, BPMI_E_ARG, "slice_n must be -1, 0 or 2^16 .. 2^23"); ctx->opt_slice_n = (int)value; return BPMI_OK; }
  if (!strcmp(name, "slice_min")) { if (value < 0 || value > (1 << 23)) return fail(ctx, BPMI_E_ARG, "slice_min must be 0 .. 2^23"); ctx->opt_slice_min = (int)value; return BPMI_OK; }
  if (!strcmp(name, "mid_parts")) { if (value < 0 || value > 4) return fail(ctx, BPMI_E_ARG, "mid_parts must be 0 .. 4"); ctx->opt_mid_parts = (int)value; msm_graphs_clear(ctx); return BPMI_OK; }
  if (!strcmp(name, "mixed_windows")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "mixed_windows must be 0 or 1"); ctx->opt_mixed = (int)value; msm_graphs_clear(ctx); return BPMI_OK; }
  if (!strcmp(name, "top_window_unsigned")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "top_window_unsigned must be 0 or 1"); ctx->opt_top2 = (int)value; msm_graphs_clear(ctx); return BPMI_OK; }
  if (!strcmp(name, "prover_table_bits")) { if (value != 0 && (value < 4 || value > 16)) return fail(ctx, BPMI_E_ARG, "prover_table_bits must be 0 or 4..16"); ctx->opt_prover_tw = (int)value; return BPMI_OK; }
  if (!strcmp(name, "ipa_fixed_generators")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "ipa_fixed_generators must be 0 or 1"); ctx->opt_ipa_fixed = (int)value; ctx->fold_key_g = ctx->fold_key_h = nullptr; return BPMI_OK; }
  if (!strcmp(name, "validate_points")) { if (value < 0 || value > 2) return fail(ctx, BPMI_E_ARG, "validate_points must be 0, 1 or 2"); ctx->opt_validate = (int)value; return BPMI_OK; }
  if (!strcmp(name, "hist_scan_fused")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "hist_scan_fused must be 0 or 1"); ctx->opt_histscan = (int)value; msm_graphs_clear(ctx); return BPMI_OK; }
  if (!strcmp(name, "reduce_fit")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "reduce_fit must be 0 or 1"); ctx->opt_reduce_fit = (int)value; msm_graphs_clear(ctx); return BPMI_OK; }
  if (!strcmp(name, "final_spread")) { if (value < 0 || value > 3) return fail(ctx, BPMI_E_ARG, "final_spread must be 0 .. 3"); ctx->opt_final_spread = (int)value; msm_graphs_clear(ctx); return BPMI_OK; }
  if (!strcmp(name, "sort_inblock")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "sort_inblock must be 0 or 1"); ctx->opt_inblock = (int)value; msm_graphs_clear(ctx); return BPMI_OK; }
  if (!strcmp(name, "segscan_fused")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "segscan_fused must be 0 or 1"); ctx->opt_segfuse = (int)value; msm_graphs_clear(ctx); return BPMI_OK; }
  if (!strcmp(name, "priority")) { if (value < 0 || value > 31 || (value > 1 && value < 16)) return fail(ctx, BPMI_E_ARG, "priority must be 0, 1 or 16 + a mask of stages"); ctx->opt_prio = (int)value; msm_graphs_clear(ctx); return BPMI_OK; }
  if (!strcmp(name, "hist_threads")) { if (value != 0 && value != 256 && value != 512 && value != 1024) return fail(ctx, BPMI_E_ARG, "hist_threads must be 0, 256, 512 or 1024"); ctx->opt_hist_threads = (int)value; return BPMI_OK; }
  if (!strcmp(name, "hist_blocks")) { if (value < 0 || value > 8192) return fail(ctx, BPMI_E_ARG, "hist_blocks must be in [0, 8192]"); ctx->opt_hist_blocks = (int)value; return BPMI_OK; }
  if (!strcmp(name, "direct_result")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "direct_result must be 0 or 1"); ctx->opt_direct = (int)value; msm_graphs_clear(ctx); return BPMI_OK; }
  if (!strcmp(name, "graphs")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "graphs must be 0 or 1"); ctx->opt_graph = (int)value; if (!value) msm_graphs_clear(ctx); return BPMI_OK; }
  if (!strcmp(name, "tail_thread")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "tail_thread must be 0 or 1"); ctx->opt_tail_thread = (int)value; return BPMI_OK; }
  if (!strcmp(name, "pair_chain")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "pair_chain must be 0 or 1"); ctx->opt_pair_chain = (int)value; return BPMI_OK; }
  if (!strcmp(name, "mid_min")) { if (value < -1 || value > MID_NMAX) return fail(ctx, BPMI_E_ARG, "mid_min must be -1 .. 8448"); ctx->opt_mid_min = (int)value; msm_graphs_clear(ctx); return BPMI_OK; }
  if (!strcmp(name, "mid_single_min")) { if (value < -1 || value > MID_NMAX) return fail(ctx, BPMI_E_ARG, "mid_single_min must be -1 .. 8448"); ctx->opt_mid_single = (int)value; msm_graphs_clear(ctx); return BPMI_OK; }
  if (!strcmp(name, "small_pair")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "small_pair must be 0 or 1"); ctx->opt_pair1 = (int)value; return BPMI_OK; }
  if (!strcmp(name, "fused_scan")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "fused_scan must be 0 or 1"); ctx->opt_fuse = (int)value; return BPMI_OK; }
  if (!strcmp(name, "quad_final")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "quad_final must be 0 or 1"); ctx->opt_quad = (int)value; return BPMI_OK; }
  if (!strcmp(name, "spin_wait")) { if (value < 0 || value > 10000000) return fail(ctx, BPMI_E_ARG, "spin_wait must be in [0, 10^7]"); ctx->opt_spin_wait = (int)value; return BPMI_OK; }
  if (!strcmp(name, "mul_batch_glv")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "mul_batch_glv must be 0 or 1"); ctx->opt_mulb = (int)value; return BPMI_OK; }
  if (!strcmp(name, "tail")) { if (value < 0 || value > 2) return fail(ctx, BPMI_E_ARG, "tail must be 0, 1 or 2"); ctx->opt_tail = (int)value; return BPMI_OK; }
  if (!strcmp(name, "small_n")) { if (value < -1 || value > (1 << 16)) return fail(ctx, BPMI_E_ARG, "small_n must be -1 .. 65536"); ctx->opt_small = (int)value; return BPMI_OK; }
  if (!strcmp(name, "split")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "split must be 0 or 1"); ctx->opt_split = (int)value; return BPMI_OK; }
  if (!strcmp(name, "async_lanes")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "async_lanes must be 0 or 1"); ctx->opt_async_lanes = (int)value; return BPMI_OK; }
  if (!strcmp(name, "rp_only_role")) { if (value < -1 || value > 3) return fail(ctx, BPMI_E_ARG, "rp_only_role must be in [-1, 3]"); ctx->opt_rp_only_role = (int)value; return BPMI_OK; }
  if (!strcmp(name, "glv")) { if (value < -1 || value > 1) return fail(ctx, BPMI_E_ARG, "glv must be -1, 0 or 1"); ctx->opt_glv = (int)value; return BPMI_OK; }
  if (!strcmp(name, "rp_priority")) { if (value < 0 || value > 2) return fail(ctx, BPMI_E_ARG, "rp_priority must be 0, 1 or 2"); ctx->opt_rp_prio = (int)value; return BPMI_OK; }
  if (!strcmp(name, "rp_slices")) { if (value < 0 || value > 4) return fail(ctx, BPMI_E_ARG, "rp_slices must be 0 .. 4"); ctx->opt_rp_slices = (int)value; return BPMI_OK; }
  if (!strcmp(name, "rp_overlap")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "rp_overlap must be 0 or 1"); ctx->opt_rp_overlap = (int)value; return BPMI_OK; }
  if (!strcmp(name, "rp_rows")) { if (value < 0) return fail(ctx, BPMI_E_ARG, "rp_rows must be >= 0"); ctx->opt_rp_rows = (int)value; return BPMI_OK; }
  if (!strcmp(name, "rp_lanes")) {
    if (value != 0 && (value < 1 || value > 64 || (value & (value - 1)))) return fail(ctx, BPMI_E_ARG, "rp_lanes must be 0 or a power of two <= 64");
    ctx->opt_rp_lanes = (int)value;
    return BPMI_OK;
  }
  if (!strcmp(name, "pair_phases")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "pair_phases must be 0 or 1"); ctx->opt_pair_phases = (int)value; return BPMI_OK; }
  if (!strcmp(name, "fold_wnaf")) { if (value < 0 || value > 2) return fail(ctx, BPMI_E_ARG, "fold_wnaf must be 0, 1 or 2"); ctx->opt_fold_wnaf = (int)value; return BPMI_OK; }
  if (!strcmp(name, "reduce_epl")) { if (value < 0 || value > 64) return fail(ctx, BPMI_E_ARG, "reduce_epl must be 0..64"); ctx->opt_epl = (int)value; return BPMI_OK; }
  if (!strcmp(name, "chunk")) { if (value < 0 || value > 4096) return fail(ctx, BPMI_E_ARG, "chunk must be 0..4096"); ctx->opt_chunk = (int)value; return BPMI_OK; }
  if (!strcmp(name, "ipa_small_step")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "ipa_small_step must be 0 or 1"); ctx->opt_ipa_step = (int)value; return BPMI_OK; }
  if (!strcmp(name, "fold_shared")) { if (value < 0 || value > 1) return fail(ctx, BPMI_E_ARG, "fold_shared must be 0 or 1"); ctx->opt_fold_shared = (int)value; return BPMI_OK; }
  if (!strcmp(name, "ipa_small_m")) { if (value < 0 || (value & (value - 1))) return fail(ctx, BPMI_E_ARG, "ipa_small_m must be 0 (default), 1 (never) or a power of two"); ctx->opt_ipa_small = value; return BPMI_OK; }
  if (!strcmp(name, "ipa_big_m")) { if (value < 0 || (value & (value - 1))) return fail(ctx, BPMI_E_ARG, "ipa_big_m must be 0 or a power of two"); ctx->opt_ipa_big = value; return BPMI_OK; }
  return fail(ctx, BPMI_E_ARG, std::string("unknown option ") + name);
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

// ---- on-curve check of caller-supplied points (option "validate_points") --------------------------------------------------
// The reference can never hand an off-curve point to multiexp: fastecdsa's Point constructor rejects it (reached from
// /root/reference/src/utils/utils.py:119-131), and ec.py keeps that check for Python callers.  A C caller hands in raw bytes, so
// the entry points that take HOST pointers check them here (level 1, the default; level 2: the synchronous _dev entry points as
// well; 0: never): the identity (64 zero bytes) or x, y < p with y^2 = x^3 + 7.  Large arrays: k_ec_validate queued behind the
// upload, its verdict (the smallest bad index) copied to a page-locked word that is read after the call's own synchronisation --
// no extra wait; the call then fails with BPMI_E_ARG and writes NO result.  A few points: checked on the host.
#define VALIDATE_HOST_MAX 64u
static int validate_begin(bpmi_ctx *ctx, hipStream_t st) {
  if (!ctx->vflag) {
    HIPCHK(ctx, hipHostMalloc((void **)&ctx->vflag, 64, hipHostMallocDefault));
    HIPCHK(ctx, hipMalloc((void **)&ctx->vflag_dev, 256));
  }
  *ctx->vflag = 0xFFFFFFFFu;
  HIPCHK(ctx, hipMemsetAsync(ctx->vflag_dev, 0xFF, 4, st));
  return BPMI_OK;
}
// array `which` (0 .. 3) of the call: d_pts[0 .. n) on the device
static void validate_enqueue(bpmi_ctx *ctx, const void *d_pts, uint64_t n, u32 which, hipStream_t st) {
  if (!n) return;
  hipLaunchKernelGGL(k_ec_validate, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, (const u32 *)d_pts, (u32)n, which << 28, ctx->vflag_dev);
}
static int validate_fetch(bpmi_ctx *ctx, hipStream_t st) {
  HIPCHK(ctx, hipMemcpyAsync(ctx->vflag, ctx->vflag_dev, 4, hipMemcpyDeviceToHost, st));
  return BPMI_OK;
}
// after the stream has been synchronised: names[which] = what the bad array is called in the message
static int validate_end(bpmi_ctx *ctx, const char *fn, const char *const *names) {
  const u32 v = *ctx->vflag;
  if (v == 0xFFFFFFFFu) return BPMI_OK;
  return fail(ctx, BPMI_E_ARG, std::string(fn) + ": " + names[v >> 28] + "[" + std::to_string(v & 0x0FFFFFFFu) + "] is not a point of the curve");
}
static int validate_host(bpmi_ctx *ctx, const uint8_t *pts, uint64_t n, const char *fn, const char *name) {
  for (uint64_t i = 0; i < n; i++) {
    u32 w[16];
    memcpy(w, pts + 64 * i, 64);
    if (!wire_point_valid(w)) return fail(ctx, BPMI_E_ARG, std::string(fn) + ": " + name + "[" + std::to_string(i) + "] is not a point of the curve");
  }
  return BPMI_OK;
}

// ---- MSM ------------------------------------------------------------------------------
static int msm_dev_impl(bpmi_ctx *ctx, const void *d_pts, const void *d_scalars, uint64_t n, uint8_t out[64]);
int bpmi_msm_dev(bpmi_ctx *ctx, const void *d_pts, const void *d_scalars, uint64_t n, uint8_t out[64]) {
  if (!ctx || !out || (n && (!d_pts || !d_scalars))) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (n > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
  if (ctx->opt_validate < 2 || n == 0) return msm_dev_impl(ctx, d_pts, d_scalars, n, out);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = validate_begin(ctx, ctx->stream);
  if (rc) return rc;
  validate_enqueue(ctx, d_pts, n, 0, ctx->stream);
  rc = validate_fetch(ctx, ctx->stream);
  if (rc) return rc;
  rc = msm_dev_impl(ctx, d_pts, d_scalars, n, out);
  if (rc) return rc;
  static const char *const names[] = {"d_pts"};
  rc = validate_end(ctx, "bpmi_msm_dev", names);
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
// Asynchronous pair: enqueue returns as soon as the MSM's kernels and its device->host copy are queued on
// the ctx stream; finish waits for THAT MSM only and runs the host part of its tail.  Two slots, so the
// host tail (and the caller's own work, e.g. the exchange of partial results) of MSM k overlaps the
// kernels of MSM k + 1.
int bpmi_msm_dev_enqueue(bpmi_ctx *ctx, int slot, const void *d_pts, const void *d_scalars, uint64_t n) {
  if (!ctx || (n && (!d_pts || !d_scalars))) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (slot < 0 || slot >= BPMI_LANES) return fail(ctx, BPMI_E_ARG, "slot must be 0, 1 or 2");
  if (n > (1ull << 23)) return fail(ctx, BPMI_E_ARG, "bpmi_msm_dev_enqueue takes at most 2^23 pairs (use bpmi_msm_dev)");
  if (ctx->opt_split) return fail(ctx, BPMI_E_STATE, "option split is not available with the asynchronous entry points");
  if (ctx->pend[slot].async) return fail(ctx, BPMI_E_STATE, "an MSM is still pending in this slot (bpmi_msm_finish it first)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Segs s = segs_init();
  s.pts[0] = (const u32 *)d_pts; s.sc[0] = (const u32 *)d_scalars; s.n[0] = (u32)n; s.total = (u32)n;
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
  rc = msm_enqueue(ctx, mode, lane, slot, s);
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
  const bool check = ctx->opt_validate >= 1;
  if (check) {
    rc = validate_begin(ctx, ctx->stream);
    if (rc) return rc;
    validate_enqueue(ctx, dp, n, 0, ctx->stream);
    rc = validate_fetch(ctx, ctx->stream);
    if (rc) return rc;
  }
  rc = msm_dev_impl(ctx, dp, ds, n, out);
  if (rc || !check) return rc;
  static const char *const names[] = {"pts"};
  rc = validate_end(ctx, "bpmi_msm", names);
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
  const bool check = ctx->opt_validate >= 1 && (n0 || n1);
  if (check) {
    rc = validate_begin(ctx, ctx->stream);
    if (rc) return rc;
    validate_enqueue(ctx, d, n0, 0, ctx->stream);
    validate_enqueue(ctx, d + o_p1, n1, 1, ctx->stream);
    rc = validate_fetch(ctx, ctx->stream);
    if (rc) return rc;
  }
  rc = msm_run_pair(ctx, a, out0, b, out1);
  if (rc || !check) return rc;
  static const char *const names[] = {"pts0", "pts1"};
  rc = validate_end(ctx, "bpmi_msm2", names);
  if (rc) { memset(out0, 0, 64); memset(out1, 0, 64); }
  return rc;
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
  const bool check = ctx->opt_validate >= 1;
  if (check) {
    rc = validate_begin(ctx, ctx->stream);
    if (rc) return rc;
    validate_enqueue(ctx, dp, n, 0, ctx->stream);
    rc = validate_fetch(ctx, ctx->stream);
    if (rc) return rc;
  }
  rc = bpmi_ec_mul_batch_dev(ctx, dp, ds, n, dout);
  if (rc) return rc;
  if (check) {                                   // the verdict before anything is written to the caller's buffer
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    static const char *const names[] = {"pts"};
    rc = validate_end(ctx, "bpmi_ec_mul_batch", names);
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
  const bool check = ctx->opt_validate >= 1;
  if (check) {
    rc = validate_begin(ctx, ctx->stream);
    if (rc) return rc;
    validate_enqueue(ctx, d1, n, 0, ctx->stream);
    validate_enqueue(ctx, d2, n, 1, ctx->stream);
    rc = validate_fetch(ctx, ctx->stream);
    if (rc) return rc;
  }
  rc = bpmi_ec_lincomb2_batch_dev(ctx, d1, d2, k1, k2, n, dout);
  if (rc) return rc;
  if (check) {
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    static const char *const names[] = {"p1", "p2"};
    rc = validate_end(ctx, "bpmi_ec_lincomb2_batch", names);
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
  const bool check = ctx->opt_validate >= 1;
  if (check && n <= VALIDATE_HOST_MAX) { rc = validate_host(ctx, pts, n, "bpmi_ec_sum", "pts"); if (rc) return rc; }
  else if (check) {
    rc = validate_begin(ctx, ctx->stream);
    if (rc) return rc;
    validate_enqueue(ctx, dp, n, 0, ctx->stream);
    rc = validate_fetch(ctx, ctx->stream);
    if (rc) return rc;
  }
  {
    StageTimer t(ctx, ST_MISC);
    hipLaunchKernelGGL(k_ec_sum, dim3(1), dim3(256), 0, ctx->stream, (const u32 *)dp, (u32)n, (u32 *)dout);
  }
  uint8_t tmp[64];
  HIPCHK(ctx, hipMemcpyAsync(tmp, dout, 64, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (check && n > VALIDATE_HOST_MAX) {
    static const char *const names[] = {"pts"};
    rc = validate_end(ctx, "bpmi_ec_sum", names);
    if (rc) return rc;
  }
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
static bool log2_exact(uint64_t n, u32 &k) { k = 0; while ((1ull << k) < n) k++; return n && (1ull << k) == n; }

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
  const bool check_host = ctx->opt_validate >= 1 && n_extra && n_extra <= VALIDATE_HOST_MAX;
  const bool check_dev = ctx->opt_validate >= 2 || (ctx->opt_validate >= 1 && n_extra > VALIDATE_HOST_MAX);
  if (check_host) { rc = validate_host(ctx, extra_pts, n_extra, "bpmi_ipa_verify_dev", "extra_pts"); if (rc) return rc; }
  if (check_dev) { rc = validate_begin(ctx, ctx->stream); if (rc) return rc; }
  rc = svector_launch(ctx, L, d_hscale, n, xs, xinvs, a, b);
  if (rc) return rc;
  u32 *d_sa = L.sa, *d_sb = L.sb;
  char *d_ex = L.extra;
  if (n_extra) {
    HIPCHK(ctx, h2d(ctx, d_ex, extra_pts, 64 * n_extra, ctx->stream));
    HIPCHK(ctx, h2d(ctx, d_ex + o_es, extra_scalars, 32 * n_extra, ctx->stream));
  }
  Segs s = segs_init();
  s.pts[0] = (const u32 *)d_g; s.sc[0] = d_sa; s.n[0] = (u32)n;
  s.pts[1] = (const u32 *)d_h; s.sc[1] = d_sb; s.n[1] = (u32)n;
  s.pts[2] = (const u32 *)d_ex; s.sc[2] = (const u32 *)(d_ex + o_es); s.n[2] = (u32)n_extra;
  s.total = (u32)(2 * n + n_extra);
  if (check_dev) {
    if (ctx->opt_validate >= 2) { validate_enqueue(ctx, d_g, n, 0, ctx->stream); validate_enqueue(ctx, d_h, n, 1, ctx->stream); }
    if (n_extra > VALIDATE_HOST_MAX) validate_enqueue(ctx, d_ex, n_extra, 2, ctx->stream);
    rc = validate_fetch(ctx, ctx->stream);
    if (rc) return rc;
  }
  rc = msm_run(ctx, s, out);
  if (rc || !check_dev) return rc;
  static const char *const names[] = {"d_g", "d_h", "extra_pts"};
  rc = validate_end(ctx, "bpmi_ipa_verify_dev", names);
  if (rc) memset(out, 0xFF, 64);                // (never the identity, which a verifier reads as "valid")
  return rc;
}

}  // extern "C"

#include "ipa_host.hpp"

extern "C" {

// ---- batch verification of range proofs: host-side preparation ---------------------------------------
int bpmi_rp_batch_prepare(uint32_t n_gens, uint32_t values_per_proof, uint64_t n_proofs, const uint8_t *blobs, uint64_t blobs_len, const uint64_t *blob_off,
                          const uint8_t *weights, const uint8_t *seed, int threads, uint8_t *v_scalars, uint8_t *pt_scalars, uint8_t *shared, uint8_t *comp_out,
                          int64_t *first_bad) {
  if (!blobs || !blob_off || (!weights && !seed) || !v_scalars || !pt_scalars || !shared || !first_bad) return BPMI_E_ARG;
  if (n_gens < 2 || (n_gens & (n_gens - 1)) || n_gens > 65536) return BPMI_E_ARG;
  const uint32_t m = values_per_proof;
  if (m < 1 || n_gens % m) return BPMI_E_ARG;
  uint32_t k = 0;
  while ((1u << k) < n_gens) k++;
  *first_bad = -1;
  // the offset table comes from the caller, the proofs from the network: never read outside blobs[0, blobs_len)
  if (blob_off[0] > blobs_len) return BPMI_E_ARG;
  for (uint64_t g = 0; g < n_proofs; g++) if (blob_off[g] > blob_off[g + 1] || blob_off[g + 1] > blobs_len) return BPMI_E_ARG;
  // wire formats 2 and 3 (rp_wire_v2_host.hpp): expanded to format 1 here (format 3's y coordinates checked), then everything below
  // runs as before
  std::vector<uint8_t> expanded;
  std::vector<uint64_t> expanded_off;
  bool any_v2 = false;
  for (uint64_t g = 0; g < n_proofs && !any_v2; g++)
    any_v2 = blob_off[g + 1] >= blob_off[g] + 5 && (blobs[blob_off[g] + 4] == '2' || blobs[blob_off[g] + 4] == '3');
  if (any_v2) {
    expanded_off.assign(n_proofs + 1, 0);
    std::vector<uint8_t> one;
    for (uint64_t g = 0; g < n_proofs; g++) {
      const uint8_t *b = blobs + blob_off[g];
      const size_t len = (size_t)(blob_off[g + 1] - blob_off[g]);
      // a format-1 proof among format-2 ones is taken as it is; so is a blob that claims format 2 and does not expand -- it is not a
      // format-1 proof either, so the checks below reject it AT ITS INDEX, behind any earlier bad proof (returning here at once made
      // the host name a later proof than the device: tools/fuzz_batch_prepare.py, round 5)
      if (len >= 5 && (b[4] == '2' || b[4] == '3') && rpw::expand_v2(b, len, one)) expanded.insert(expanded.end(), one.begin(), one.end());
      else expanded.insert(expanded.end(), b, b + len);
      expanded_off[g + 1] = expanded.size();
    }
    blobs = expanded.data(); blobs_len = expanded.size(); blob_off = expanded_off.data();
  }
  const size_t nacc = 5 + 2 * (size_t)n_gens;
  if (threads < 1) threads = 1;
  if ((uint64_t)threads > n_proofs) threads = n_proofs ? (int)n_proofs : 1;
  std::vector<uint64_t> pt_off(n_proofs + 1);
  for (uint64_t g = 0; g <= n_proofs; g++) pt_off[g] = g * (6 + 2 * (uint64_t)k);
  std::vector<std::vector<rp::Sq>> acc(threads, std::vector<rp::Sq>(nacc, rp::q_small(0)));
  std::vector<uint64_t> bad(threads, UINT64_MAX);
  auto work = [&](int t) {
    const uint64_t lo = n_proofs * t / threads, hi = n_proofs * (t + 1) / threads;
    // sub-chunks bound the scratch memory and keep one modular inversion per ~512 proofs
    for (uint64_t a = lo; a < hi; a += 512) {
      const uint64_t b = a + 512 < hi ? a + 512 : hi;
      uint64_t bd = UINT64_MAX;
      if (!rp::run_chunk(n_gens, k, m, blobs, blob_off, weights, a, b, pt_off.data(), v_scalars, pt_scalars, comp_out, acc[t].data(), &bd, seed)) { bad[t] = bd; return; }
    }
  };
  if (threads == 1) work(0);
  else {
    std::vector<std::thread> th;
    for (int t = 0; t < threads; t++) th.emplace_back(work, t);
    for (auto &x : th) x.join();
  }
  for (int t = 0; t < threads; t++) if (bad[t] != UINT64_MAX && (*first_bad < 0 || (int64_t)bad[t] < *first_bad)) *first_bad = (int64_t)bad[t];
  for (size_t i = 0; i < nacc; i++) {
    rp::Sq sum = rp::q_small(0);
    for (int t = 0; t < threads; t++) rp::q_add(sum, sum, acc[t][i]);
    rp::q_to_le(shared + 32 * i, sum);
  }
  return BPMI_OK;
}

// The same preparation on the GPU (rp_batch_kernels.hpp): the wire proofs are uploaded (in a few slices, so that the decoding of
// the points of slice c runs on the second lane while slice c + 1 is still on the link), one lane per proof and role parses,
// hashes and checks them, the weighted scalars are written straight into the caller's device scalar arrays, the proofs' points
// are decoded where they lie in the blobs into d_points, and only the (5 + 2n) shared coefficients and the verdict come back.
struct RpQueued { u32 *d_shared; unsigned long long *d_bad; u32 ncols; };
// bpmi_rp_batch_group_values_dev: the preparation sums the cells per GROUP of `group` proofs instead of per batch and leaves one verdict
// byte per proof (k_rp_verdict, k_rp_group_colsum); the arrays live behind the preparation's own in ctx->rp_buf
struct RpGroups {
  u32 group, ngroups;        // in
  u32 *d_gsum, *d_gfin;      // out: ngroups x (5 + 2n) raw column sums; room for the ngroups x (3 + 2n) scalars of the groups' MSMs
  uint8_t *d_verdict, *d_ptflag;
  u32 *d_E, *d_vals;         // room for the window sums (37 per group) and the 64-byte values
};
#define RP_UPLOAD_SLICES 4
// A batch is read in the wire format of its FIRST proof.  A well-formed proof of the OTHER format inside it is not a forged proof: the
// device paths report it as an argument error ("mixed wire formats"), not as a verdict -- a verifier must be able to tell a
// sender's mix-up from an attack (the host path, bpmi_rp_batch_prepare, takes the formats proof by proof).
static int rp_mixed_formats(bpmi_ctx *ctx, const uint8_t *blobs, uint64_t blobs_len, const uint64_t *blob_off, int64_t first_bad) {
  if (first_bad < 0) return BPMI_OK;
  const uint64_t a0 = blob_off[0], a = blob_off[first_bad], e = blob_off[first_bad + 1];
  if (a0 + 5 > blobs_len || e > blobs_len || e < a + 5) return BPMI_OK;
  const uint8_t *b = blobs + a;
  const uint8_t call = (blobs[a0 + 4] == '2' || blobs[a0 + 4] == '3') ? blobs[a0 + 4] : (uint8_t)'1';
  if (!(b[0] == 'B' && b[1] == 'P' && b[2] == 'R' && b[3] == 'P' && b[4] >= '1' && b[4] <= '3' && b[4] != call)) return BPMI_OK;
  // WELL-FORMED in the format it claims?  (a format-1 proof whose magic a flipped bit turned into "BPRP3" is a bad proof, not a mix-up)
  const size_t len = (size_t)(e - a);
  rp::Parsed parsed;
  const bool well_formed = b[4] == '1' ? rp::parse_blob(parsed, b, len) : (len > 0 && rpw::v2_length(b, len) == len);
  if (well_formed)
    return fail(ctx, BPMI_E_ARG, "mixed wire formats: proof " + std::to_string(first_bad) + " is format " + std::string(1, (char)b[4]) + " in a format-" +
                                     std::string(1, (char)call) + " batch (one format per call; bpmi_rp_wire_v2_to_v1 converts)");
  return BPMI_OK;
}
// queues everything on the ctx's two lanes and returns without waiting; the results stay on the device (d_shared: 5 + 2n
// scalars of 8 words, *d_bad behind them).  The caller waits for both lanes whatever this returns.
static int rp_prepare_enqueue(bpmi_ctx *ctx, uint32_t n_gens, uint32_t m, uint64_t n_proofs, const uint8_t *blobs, uint64_t blobs_len, const uint64_t *blob_off,
                              const uint8_t *weights, const uint8_t *seed, void *d_v_scalars, void *d_pt_scalars, void *d_points, RpQueued &Q,
                              RpGroups *G = nullptr) {
  if (n_gens < 2 || (n_gens & (n_gens - 1)) || n_gens > 65536) return fail(ctx, BPMI_E_ARG, "n_gens must be a power of two in [2, 65536]");
  if (m < 1 || n_gens % m) return fail(ctx, BPMI_E_ARG, "values_per_proof must divide n_gens");
  if (n_proofs == 0 || n_proofs > (1ull << 22)) return fail(ctx, BPMI_E_ARG, "n_proofs must be in [1, 2^22]");
  if (blobs_len > (1ull << 32)) return fail(ctx, BPMI_E_ARG, "at most 4 GiB of proofs per call");
  uint32_t k = 0;
  while ((1u << k) < n_gens) k++;
  if (blob_off[0] > blobs_len) return fail(ctx, BPMI_E_ARG, "offset table leaves the buffer");
  // wire format 2 (rp_wire_v2_host.hpp): told by the first proof's magic; every proof of the call must then be format 2 (the device
  // expander refuses the others).  The array the roles read holds the EXPANDED proofs: its rows are sized by the longest expansion
  const uint8_t fmt0 = (blob_off[1] >= blob_off[0] + 5 && blob_off[0] + 5 <= blobs_len) ? blobs[blob_off[0] + 4] : (uint8_t)'1';
  const bool v2 = fmt0 == '2' || fmt0 == '3';
  const uint64_t hint_bytes = fmt0 == '3' ? 32ull * (6 + 2 * k) : 0;             // format 3: the points' y coordinates behind the format-2 proof
  // The expander, the roles and the element kernel are chains of dependent instructions, one wave per SIMD; on formats 1 and 2 they run beside
  // the second lane's square roots (k_ec_decompress_wire: every issue slot it can get).  Raised issue priority lets the chains run at their
  // own speed: format 2 alone 1.71-1.73 -> 1.64-1.68 ms, ten in flight +2.4-2.8 % (two boxes, profiles/r06_C5_preparation_priority_ab.txt);
  // format 3 has no square roots beside it and gains nothing (option "rp_priority": 0 off, 1 = formats 1 and 2 (default), 2 = always)
  const u32 rp_prio = (ctx->opt_rp_prio == 2 || (ctx->opt_rp_prio == 1 && fmt0 != '3')) ? 1u : 0u;
  uint64_t maxlen = 0;
  for (uint64_t g = 0; g < n_proofs; g++) {
    if (blob_off[g] > blob_off[g + 1] || blob_off[g + 1] > blobs_len) return fail(ctx, BPMI_E_ARG, "offset table leaves the buffer");
    uint64_t len = blob_off[g + 1] - blob_off[g];
    if (v2) {
      // longest expansion a format-2 proof of this length can have (its seeds' lengths are NOT read here: 2^14 scattered reads of
      // the receive buffer cost more than the upload saves): S seed bytes in all, base64 of them at most three times (the
      // Protocol-1 seed appears in two transcripts), every point item 45 bytes, every decimal item 79
      const uint64_t body = 6 + 32ull * (5 + k) + 33ull * (6 + 2 * k);
      const uint64_t S = len > body + 132 + hint_bytes ? len - body - 132 - hint_bytes : 0;
      len = body + 2 + 12 + 3 * (4 * ((S + 2) / 3) + 1) + 4 * 45 + 3 * 79 + 2 * 79 + 1 + (uint64_t)k * (45 + 45 + 79);
    }
    maxlen = std::max(maxlen, len);
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const u32 P = (u32)n_proofs, ncols = 5 + 2 * n_gens, per = 6 + 2 * k;
  // the proofs as 8-byte words, word-major (k_rp_transpose): W rows of P words, 16 rows of zero padding for loads that run past a proof
  const u32 W = (u32)((std::min<uint64_t>(maxlen, RP_MAX_PROOF_BYTES) + 7) / 8) + 16;
  // device staging: blobs | offsets | weights | status
  const size_t o_off = align_up(blobs_len + 128, 256);      // 128 bytes of slack: the kernel's batched 8-byte loads may run past the last proof
  const size_t o_w = o_off + align_up(8 * ((size_t)P + 1), 256), o_st = o_w + (weights ? align_up(128 * (size_t)P, 256) : 0);
  int rc = ensure_stage_in(ctx, o_st + align_up(RP_ROLES * (size_t)P, 256));
  if (rc) return rc;
  rc = ensure_lane(ctx, 1);
  if (rc) return rc;
  rc = ensure_pin(ctx, 32 * (size_t)ncols + 64);
  if (rc) return rc;
  for (int c = 0; c < RP_UPLOAD_SLICES; c++)
    if (!ctx->ev_slice[c]) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_slice[c], hipEventDisableTiming));
  char *din = (char *)ctx->stage_in;
  // contributions + contexts: at most ~256 MB of cells per launch
  const u32 nslots = CTX_SLOTS(k, m);
  const size_t cell_row = 36 * ((size_t)ncols + nslots), out_row = 32 * (size_t)ncols;       // scratch cells are 9 limbs, the result 8 words
  u32 rows = (u32)std::min<size_t>(P, std::max<size_t>(1, ((size_t)256 << 20) / cell_row));
  if (ctx->opt_rp_rows > 0) rows = std::min<u32>(rows, (u32)ctx->opt_rp_rows);
  const size_t o_ctx = align_up(36 * (size_t)ncols * rows, 256), o_shared = o_ctx + align_up(36 * (size_t)nslots * rows, 256),
               o_T = o_shared + align_up(2 * out_row + 256, 256), T_bytes = 8 * (size_t)W * P,      // summed columns | verdict | MSM scalars of the shared generators
               o_lens = o_T + align_up(T_bytes, 256);                                               // format 2: lengths of the expanded proofs
  size_t need = o_lens + 4 * (size_t)P + 256;
  size_t o_gsum = 0, o_gfin = 0, o_verdict = 0, o_ptflag = 0, o_E = 0, o_vals = 0;
  if (G) {
    const size_t ng = G->ngroups;
    o_gsum = align_up(need, 256); o_gfin = o_gsum + align_up(32 * (size_t)ncols * ng, 256);
    o_verdict = o_gfin + align_up(32 * (size_t)(ncols - 2) * ng, 256); o_ptflag = o_verdict + align_up(P, 256);
    o_E = o_ptflag + align_up(P, 256); o_vals = o_E + align_up(4ull * XYZZ_WORDS * (255u / MID_C + 1u) * ng, 256);
    need = o_vals + 64 * ng + 256;
  }
  if (need > ctx->rp_buf_bytes) {
    if (ctx->rp_buf) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(ctx->rp_buf)); ctx->rp_buf = nullptr; ctx->rp_buf_bytes = 0; }
    HIPCHK(ctx, hipMalloc(&ctx->rp_buf, need));
    ctx->rp_buf_bytes = need;
  }
  u32 *d_contrib = (u32 *)ctx->rp_buf, *d_ctx = (u32 *)((char *)ctx->rp_buf + o_ctx), *d_shared = (u32 *)((char *)ctx->rp_buf + o_shared);
  u64 *d_T = (u64 *)((char *)ctx->rp_buf + o_T);
  unsigned long long *d_bad = (unsigned long long *)(d_shared + 8 * (size_t)ncols);
  Q.d_shared = d_shared; Q.d_bad = d_bad; Q.ncols = ncols;
  HIPCHK(ctx, h2d(ctx, din + o_off, blob_off, 8 * ((size_t)P + 1), ctx->stream));
  if (weights) HIPCHK(ctx, h2d(ctx, din + o_w, weights, 128 * (size_t)P, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(d_shared, 0, out_row, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(d_bad, 0xFF, 8, ctx->stream));
  if (G) {
    char *b = (char *)ctx->rp_buf;
    G->d_gsum = (u32 *)(b + o_gsum); G->d_gfin = (u32 *)(b + o_gfin); G->d_verdict = (uint8_t *)(b + o_verdict); G->d_ptflag = (uint8_t *)(b + o_ptflag);
    G->d_E = (u32 *)(b + o_E); G->d_vals = (u32 *)(b + o_vals);
    HIPCHK(ctx, hipMemsetAsync(G->d_gsum, 0, 32 * (size_t)ncols * G->ngroups, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(G->d_ptflag, 0, P, ctx->stream));            // (before the slices' events: the second lane's decoding sets flags)
  }
  // Upload in slices of whole proofs; the point decoding of a slice (second lane; it reads only the wire bytes) starts as soon as the
  // slice has arrived and runs beside the upload of the next one and, for the last slice, beside the preparation kernels.
  // Option rp_overlap = 0 (measurements only): one decoding launch BEHIND the preparation kernels on the same stream, so that
  // every kernel's duration is its own.
  auto decode = [&](hipStream_t st, u32 g0, u32 g1) {
    StageTimer t(ctx, ST_DECOMP, st);
    const u64 npts = (u64)(g1 - g0) * per;
    hipLaunchKernelGGL(k_ec_decompress_wire, dim3((u32)((npts + 255) / 256)), dim3(256), 0, st, (const uint8_t *)din, (const u64 *)(din + o_off) + g0,
                       k, g1 - g0, (u64)g0, (u32)RP_MAX_PROOF_BYTES, (u32 *)d_points + 16ull * per * g0, d_bad, G ? G->d_ptflag + g0 : (uint8_t *)nullptr);
  };
  // (format 3's points are checked, not computed: 0.02 ms for 2^14 proofs -- nothing to hide behind an upload, and four uploads with their
  // events cost more than one: a batch alone 1.63 ms against 1.72; the one check still runs on the second lane, beside the expander)
  const u32 nsl = (P >= 4096 && ctx->opt_rp_overlap) ? (ctx->opt_rp_slices > 0 ? (u32)ctx->opt_rp_slices : (fmt0 != '3' ? RP_UPLOAD_SLICES : 1u)) : 1u;
  for (u32 c = 0; c < nsl; c++) {
    const u32 g0 = (u32)((uint64_t)P * c / nsl), g1 = (u32)((uint64_t)P * (c + 1) / nsl);
    const uint64_t b0 = c == 0 ? 0 : blob_off[g0], b1 = c + 1 == nsl ? blobs_len : blob_off[g1];
    if (b1 > b0) HIPCHK(ctx, h2d(ctx, din + b0, blobs + b0, b1 - b0, ctx->stream));
    if (ctx->opt_rp_overlap) {
      HIPCHK(ctx, hipEventRecord(ctx->ev_slice[c], ctx->stream));
      HIPCHK(ctx, hipStreamWaitEvent(ctx->lane[1].stream, ctx->ev_slice[c], 0));
      decode(ctx->lane[1].stream, g0, g1);
    }
  }
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipEventRecord(ctx->ev_join, ctx->lane[1].stream));
  u32 *d_lens = v2 ? (u32 *)((char *)ctx->rp_buf + o_lens) : nullptr;
  if (v2) {
    // the expander writes the format-1 proofs word-major itself; what it does not write must read as zero
    HIPCHK(ctx, hipMemsetAsync(d_T, 0, T_bytes, ctx->stream));
    StageTimer t(ctx, ST_RPPREP);
    hipLaunchKernelGGL(rpd::k_rp_expand_v2, dim3((P + 3) / 4), dim3(64), 0, ctx->stream, (const uint8_t *)din, (const u64 *)(din + o_off), P, k, W, d_T, d_lens,
                       (u32)fmt0, rp_prio);
  } else {
    StageTimer t(ctx, ST_RPPREP);
    hipLaunchKernelGGL(rpd::k_rp_transpose, dim3((P + 63) / 64, (W + 63) / 64), dim3(256), 0, ctx->stream, (const uint8_t *)din, (const u64 *)(din + o_off), P, W, d_T);
  }
  rpd::Params q;
  q.Tstride = P;
  q.weights = weights ? (const uint8_t *)(din + o_w) : nullptr;
  for (int i = 0; i < 8; i++) q.seed[i] = seed ? ((u32)seed[4 * i] << 24) | ((u32)seed[4 * i + 1] << 16) | ((u32)seed[4 * i + 2] << 8) | seed[4 * i + 3] : 0;
  q.n = n_gens; q.k = k; q.m = m; q.Pall = P; q.only_role = ctx->opt_rp_only_role;
  q.contrib = d_contrib;
  q.prio = rp_prio;
  q.ctx = d_ctx;
  q.bad = d_bad;
  const size_t lds_bytes = ((size_t)k + 1) * 9 * 64 * sizeof(u32);            // role 2: k + 1 prefix products of 9 limbs per lane
  u32 lb = 0;
  while ((1u << lb) < n_gens / m) lb++;
  rpd::ElemGeom eg;
  eg.el_log = std::min<u32>(3u, lb);
  eg.ranges = n_gens >> eg.el_log;
  // groups: the per-proof verdict needs the point flags, so the decoding comes first (no overlap: queued here; else the join below)
  if (G && !ctx->opt_rp_overlap) decode(ctx->stream, 0, P);
  for (u32 base = 0; base < P; base += rows) {
    const u32 cnt = std::min(rows, P - base);
    u32 lanes = (u32)ctx->opt_rp_lanes;
    if (!lanes) lanes = 64;
    q.off = (const u64 *)(din + o_off) + base;
    q.lens = v2 ? d_lens + base : nullptr;
    q.T = d_T + base;
    q.P = cnt; q.lanes = lanes; q.first = base;
    q.v_scalars = (u32 *)d_v_scalars + 8 * (size_t)base * m;
    q.pt_scalars = (u32 *)d_pt_scalars + 8 * (size_t)base * per;
    q.status = (uint8_t *)(din + o_st) + base;
    {
      StageTimer t(ctx, ST_RPPREP);
      hipLaunchKernelGGL(rpd::k_rp_roles, dim3(RP_ROLES * ((cnt + lanes - 1) / lanes)), dim3(64), lds_bytes, ctx->stream, q);
    }
    {
      StageTimer t(ctx, ST_RPELEM);
      hipLaunchKernelGGL(rpd::k_rp_elements, dim3(2 * eg.ranges * ((cnt + 63) / 64)), dim3(64), 0, ctx->stream, q, eg);
      if (!G) hipLaunchKernelGGL(rpd::k_rp_colsum, dim3(ncols), dim3(256), 0, ctx->stream, (const u32 *)d_contrib, cnt, d_shared);
    }
    if (G) {
      if (base == 0 && ctx->opt_rp_overlap) HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));      // the two lanes join: every point flag is set
      StageTimer t(ctx, ST_RPELEM);
      rpd::VerdictArgs va;
      va.role_status = (const uint8_t *)(din + o_st); va.pt_flag = G->d_ptflag; va.verdict = G->d_verdict;
      va.Pall = P; va.first = base; va.cnt = cnt; va.m = m; va.per = per; va.only_role = ctx->opt_rp_only_role;
      va.v_scalars = (u32 *)d_v_scalars; va.pt_scalars = (u32 *)d_pt_scalars; va.points = (u32 *)d_points;
      hipLaunchKernelGGL(rpd::k_rp_verdict, dim3((u32)(((uint64_t)cnt * (m + per) + 255) / 256)), dim3(256), 0, ctx->stream, va);
      const u32 t0 = base / G->group, nt = (base + cnt - 1) / G->group - t0 + 1;                  // the groups with proofs in this chunk
      u32 lpg = 1;
      while (lpg < 64u && lpg < G->group) lpg <<= 1;
      const u32 gpb = 64u / lpg, nblk = (nt + gpb - 1) / gpb;
      hipLaunchKernelGGL(rpd::k_rp_group_colsum, dim3(ncols * nblk), dim3(64), 0, ctx->stream, (const u32 *)d_contrib, cnt, base, (const uint8_t *)G->d_verdict,
                         G->group, t0, nt, lpg, ncols, G->d_gsum);
    }
  }
  if (!ctx->opt_rp_overlap && !G) decode(ctx->stream, 0, P);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
  return BPMI_OK;
}
// both lanes idle again; the first error of (rc, the two waits)
static int rp_wait_lanes(bpmi_ctx *ctx, int rc) {
  const hipError_t e0 = wait_stream(ctx, ctx->stream), e1 = ctx->lane[1].stream ? wait_stream(ctx, ctx->lane[1].stream) : hipSuccess;      // (lane 2 never takes part in a batch)
  if (rc) return rc;
  HIPCHK(ctx, e0);
  HIPCHK(ctx, e1);
  return BPMI_OK;
}
int bpmi_rp_batch_prepare_dev(bpmi_ctx *ctx, uint32_t n_gens, uint32_t values_per_proof, uint64_t n_proofs, const uint8_t *blobs, uint64_t blobs_len,
                              const uint64_t *blob_off, const uint8_t *weights, const uint8_t *seed, void *d_v_scalars, void *d_pt_scalars, void *d_points,
                              uint8_t *shared, int64_t *first_bad) {
  if (!ctx) return BPMI_E_ARG;
  if (!blobs || !blob_off || (!weights && !seed) || !d_v_scalars || !d_pt_scalars || !d_points || !shared || !first_bad) return fail(ctx, BPMI_E_ARG, "null argument");
  *first_bad = -1;
  RpQueued Q;
  int rc = rp_prepare_enqueue(ctx, n_gens, values_per_proof, n_proofs, blobs, blobs_len, blob_off, weights, seed, d_v_scalars, d_pt_scalars, d_points, Q);
  const size_t out_row = rc ? 0 : 32 * (size_t)Q.ncols;
  if (!rc && hipMemcpyAsync(ctx->pin, Q.d_shared, out_row + 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = fail(ctx, BPMI_E_HIP, "copy of the shared coefficients failed");
  // an error in the middle must not return while the second lane is still writing into the caller's point array
  rc = rp_wait_lanes(ctx, rc);
  if (rc) return rc;
  memcpy(shared, ctx->pin, out_row);
  unsigned long long bad;
  memcpy(&bad, (char *)ctx->pin + out_row, 8);
  *first_bad = bad == ~0ull ? -1 : (int64_t)bad;
  rc = rp_mixed_formats(ctx, blobs, blobs_len, blob_off, *first_bad);
  if (rc) return rc;
  if (ctx->opt_rp_only_role >= 0) *first_bad = 0;        // a profiling run checked part of every proof: it must never read as "all valid"
  return BPMI_OK;
}

// The whole batch verification in ONE call: preparation as above, the shared coefficients folded on the device into the scalars of
// the 3 + 2n shared generators (k_rp_shared_scalars), and the batch's one MSM over [shared generators | commitments | proof
// points] -- no host round trip between the preparation and the MSM.  out = the 64-byte value of the combination (the identity
// for a valid batch; a sharded caller folds the ranks' values), *first_bad as above (then `out` means nothing).
//   v_points  HOST, n_proofs x values_per_proof x 64 B: the commitments, in proof order
//   d_gens    DEVICE, (3 + 2 n_gens) x 64 B: g, h, u, gs, hs (uploaded once per verifier)
//   d_points  DEVICE scratch, (n_proofs (values_per_proof + 6 + 2k)) x 64 B;  d_scalars  DEVICE scratch, the same count x 32 B
int bpmi_rp_batch_verify_dev(bpmi_ctx *ctx, uint32_t n_gens, uint32_t values_per_proof, uint64_t n_proofs, const uint8_t *blobs, uint64_t blobs_len,
                             const uint64_t *blob_off, const uint8_t *weights, const uint8_t *seed, const uint8_t *v_points, const void *d_gens, void *d_points,
                             void *d_scalars, uint8_t out[64], int64_t *first_bad) {
  if (!ctx) return BPMI_E_ARG;
  if (!blobs || !blob_off || (!weights && !seed) || !v_points || !d_gens || !d_points || !d_scalars || !out || !first_bad) return fail(ctx, BPMI_E_ARG, "null argument");
  *first_bad = -1;
  uint32_t k = 0;
  while ((1u << k) < n_gens) k++;
  const uint64_t nv = n_proofs * values_per_proof, npts = n_proofs * (6 + 2 * (uint64_t)k);
  if (3 + 2 * (uint64_t)n_gens + nv + npts > (1ull << 23)) return fail(ctx, BPMI_E_ARG, "at most 2^23 points in the batch's MSM");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // commitments: the first nv points / scalars of the per-proof arrays
  HIPCHK(ctx, h2d(ctx, d_points, v_points, 64 * nv, ctx->stream));
  const bool check = ctx->opt_validate >= 1;
  if (check) {
    int vrc = validate_begin(ctx, ctx->stream);
    if (vrc) return vrc;
    validate_enqueue(ctx, d_points, nv, 0, ctx->stream);
    if (ctx->opt_validate >= 2) validate_enqueue(ctx, d_gens, 3 + 2 * (uint64_t)n_gens, 1, ctx->stream);
    vrc = validate_fetch(ctx, ctx->stream);
    if (vrc) return vrc;
  }
  RpQueued Q;
  int rc = rp_prepare_enqueue(ctx, n_gens, values_per_proof, n_proofs, blobs, blobs_len, blob_off, weights, seed, d_scalars, (char *)d_scalars + 32 * nv,
                              (char *)d_points + 64 * nv, Q);
  u32 *d_fin = nullptr;
  if (!rc) {
    // scalars of g, h, u, gs_i, hs_i: c_g, c_h, c_u, c_gs[i] + gs_const, c_hs[i] + hs_const -- in place behind the raw sums
    d_fin = Q.d_shared + 8 * (size_t)Q.ncols + 32;
    {
      StageTimer t(ctx, ST_RPELEM);
      hipLaunchKernelGGL(rpd::k_rp_shared_scalars, dim3((3 + 2 * n_gens + 255) / 256), dim3(256), 0, ctx->stream, (const u32 *)Q.d_shared, n_gens, d_fin);
    }
    if (hipMemcpyAsync(ctx->pin, Q.d_bad, 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = fail(ctx, BPMI_E_HIP, "copy of the verdict failed");
  }
  if (rc) return rp_wait_lanes(ctx, rc);
  Segs s = segs_init();
  s.pts[0] = (const u32 *)d_gens; s.sc[0] = d_fin; s.n[0] = 3 + 2 * n_gens;
  s.pts[1] = (const u32 *)d_points; s.sc[1] = (const u32 *)d_scalars; s.n[1] = (u32)(nv + npts);
  s.total = s.n[0] + s.n[1];
  rc = msm_run(ctx, s, out);                      // waits for the MSM (ctx stream: behind everything queued above)
  rc = rp_wait_lanes(ctx, rc);
  if (rc) return rc;
  if (check) {
    static const char *const names[] = {"v_points", "d_gens"};
    rc = validate_end(ctx, "bpmi_rp_batch_verify_dev", names);
    if (rc) { memset(out, 0xFF, 64); return rc; }                  // (never the identity)
  }
  unsigned long long bad;
  memcpy(&bad, ctx->pin, 8);
  *first_bad = bad == ~0ull ? -1 : (int64_t)bad;
  rc = rp_mixed_formats(ctx, blobs, blobs_len, blob_off, *first_bad);
  if (rc) { memset(out, 0xFF, 64); return rc; }
  if (ctx->opt_rp_only_role >= 0) *first_bad = 0;
  return BPMI_OK;
}
// Which proofs of a rejected batch are the bad ones (replaces what a caller of the reference gets from verifying one proof at a time:
// src/rangeproofs/rangeproof_verifier.py:55-99, rangeproof_aggreg_verifier.py:55-108): the preparation of bpmi_rp_batch_verify_dev, but the
// cells are summed per GROUP of `group` consecutive proofs, the groups' MSMs over [shared generators | the group's commitments | the
// group's proof points] run as ONE launch over (group, window) (k_msm_group) with a device tail (k_group_tail), and every proof gets a
// verdict byte for its byte-level checks.  values[t] = the 64-byte value of group t's combination over its UNFLAGGED proofs (64 zero
// bytes: all of them verify); status[i] = bit 0: a byte-level check failed (parse, transcript, scalar range) | bit 1: an invalid point
// encoding.  A flagged proof contributes to no group.  A group whose MSM does not fit the one-launch kernel (3 + 2n + group (m + 6 + 2k) >
// MID_NMAX pairs) goes through msm_run, group by group: the same 64 bytes.
int bpmi_rp_batch_group_values_dev(bpmi_ctx *ctx, uint32_t n_gens, uint32_t values_per_proof, uint64_t n_proofs, const uint8_t *blobs, uint64_t blobs_len,
                                   const uint64_t *blob_off, const uint8_t *weights, const uint8_t *seed, const uint8_t *v_points, const void *d_gens,
                                   void *d_points, void *d_scalars, uint64_t group, uint8_t *values, uint8_t *status) {
  if (!ctx) return BPMI_E_ARG;
  if (!blobs || !blob_off || (!weights && !seed) || !v_points || !d_gens || !d_points || !d_scalars || !values || !status) return fail(ctx, BPMI_E_ARG, "null argument");
  if (group < 1) return fail(ctx, BPMI_E_ARG, "group must be at least 1");
  if (n_proofs == 0 || n_proofs > (1ull << 22)) return fail(ctx, BPMI_E_ARG, "n_proofs must be in [1, 2^22]");
  uint32_t k = 0;
  while ((1u << k) < n_gens) k++;
  const uint32_t m = values_per_proof, per = 6 + 2 * k, nshared = 3 + 2 * n_gens;
  const uint64_t nv = n_proofs * m, npts = n_proofs * per;
  if (nshared + nv + npts > (1ull << 23)) return fail(ctx, BPMI_E_ARG, "at most 2^23 points in the batch's MSM");
  RpGroups G;
  memset(&G, 0, sizeof(G));
  G.group = (u32)std::min<uint64_t>(group, n_proofs);
  G.ngroups = (u32)((n_proofs + G.group - 1) / G.group);
  if ((uint64_t)G.ngroups * nshared > (1ull << 26)) return fail(ctx, BPMI_E_ARG, "too many groups: n_groups x (3 + 2 n_gens) must not exceed 2^26");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t vals_bytes = 64 * (size_t)G.ngroups;
  int rc = ensure_pin(ctx, std::max<size_t>(32 * (size_t)(5 + 2 * n_gens) + 64, vals_bytes + n_proofs + 64));
  if (rc) return rc;
  HIPCHK(ctx, h2d(ctx, d_points, v_points, 64 * nv, ctx->stream));
  const bool check = ctx->opt_validate >= 1;
  if (check) {
    int vrc = validate_begin(ctx, ctx->stream);
    if (vrc) return vrc;
    validate_enqueue(ctx, d_points, nv, 0, ctx->stream);
    if (ctx->opt_validate >= 2) validate_enqueue(ctx, d_gens, nshared, 1, ctx->stream);
    vrc = validate_fetch(ctx, ctx->stream);
    if (vrc) return vrc;
  }
  RpQueued Q;
  rc = rp_prepare_enqueue(ctx, n_gens, m, n_proofs, blobs, blobs_len, blob_off, weights, seed, d_scalars, (char *)d_scalars + 32 * nv, (char *)d_points + 64 * nv, Q, &G);
  if (rc) return rp_wait_lanes(ctx, rc);
  {
    StageTimer t(ctx, ST_RPELEM);
    hipLaunchKernelGGL(rpd::k_rp_group_scalars, dim3((u32)(((uint64_t)G.ngroups * nshared + 255) / 256)), dim3(256), 0, ctx->stream, (const u32 *)G.d_gsum, n_gens,
                       G.ngroups, G.d_gfin);
  }
  const uint64_t pairs = nshared + (uint64_t)G.group * (m + per);          // of a full group
  const u32 W = 255u / MID_C + 1u;
  if (pairs <= MID_NMAX) {
    GroupMsm J;
    J.gens = (const u32 *)d_gens; J.gsc = G.d_gfin;
    J.v_pts = (const u32 *)d_points; J.v_sc = (const u32 *)d_scalars;
    J.p_pts = (const u32 *)d_points + 16 * nv; J.p_sc = (const u32 *)d_scalars + 8 * nv;
    J.nshared = nshared; J.m = m; J.per = per; J.group = G.group; J.P = (u32)n_proofs; J.W = W; J.E = G.d_E;
    {
      StageTimer t(ctx, ST_ACCUM);
      if (pairs <= GROUP_LIGHT_NMAX) hipLaunchKernelGGL((k_msm_group<GROUP_LIGHT_THREADS, GROUP_LIGHT_NMAX>), dim3(G.ngroups * W), dim3(GROUP_LIGHT_THREADS), 0, ctx->stream, J);
      else hipLaunchKernelGGL((k_msm_group<MID_THREADS, MID_NMAX>), dim3(G.ngroups * W), dim3(MID_THREADS), 0, ctx->stream, J);
      hipLaunchKernelGGL(k_group_tail, dim3((G.ngroups + 63) / 64), dim3(64), 0, ctx->stream, (const u32 *)G.d_E, W, (u32)MID_C, G.ngroups, G.d_vals);
    }
    if (hipGetLastError() != hipSuccess) rc = fail(ctx, BPMI_E_HIP, "launch of the group MSMs failed");
    if (!rc && hipMemcpyAsync(ctx->pin, G.d_vals, vals_bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = fail(ctx, BPMI_E_HIP, "copy of the group values failed");
  }
  if (!rc && hipMemcpyAsync((char *)ctx->pin + vals_bytes, G.d_verdict, n_proofs, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
    rc = fail(ctx, BPMI_E_HIP, "copy of the verdicts failed");
  rc = rp_wait_lanes(ctx, rc);
  if (rc) return rc;
  memcpy(status, (char *)ctx->pin + vals_bytes, n_proofs);
  if (pairs <= MID_NMAX) {
    memcpy(values, ctx->pin, vals_bytes);
  } else {
    // groups beyond the one-launch kernel's capacity: one MSM each on the three segments
    for (u32 t = 0; t < G.ngroups && !rc; t++) {
      const uint64_t g0 = (uint64_t)t * G.group, cnt = std::min<uint64_t>(G.group, n_proofs - g0);
      Segs s = segs_init();
      s.pts[0] = (const u32 *)d_gens; s.sc[0] = G.d_gfin + 8 * (size_t)nshared * t; s.n[0] = nshared;
      s.pts[1] = (const u32 *)d_points + 16 * m * g0; s.sc[1] = (const u32 *)d_scalars + 8 * m * g0; s.n[1] = (u32)(cnt * m);
      s.pts[2] = (const u32 *)d_points + 16 * (nv + per * g0); s.sc[2] = (const u32 *)d_scalars + 8 * (nv + per * g0); s.n[2] = (u32)(cnt * per);
      s.total = s.n[0] + s.n[1] + s.n[2];
      rc = msm_run(ctx, s, values + 64 * (size_t)t);
    }
    rc = rp_wait_lanes(ctx, rc);
    if (rc) { memset(values, 0xFF, vals_bytes); return rc; }
  }
  if (check) {
    static const char *const names[] = {"v_points", "d_gens"};
    rc = validate_end(ctx, "bpmi_rp_batch_group_values_dev", names);
    if (rc) { memset(values, 0xFF, vals_bytes); return rc; }
  }
  int64_t first_flagged = -1;
  for (uint64_t i = 0; i < n_proofs && first_flagged < 0; i++) if (status[i]) first_flagged = (int64_t)i;
  rc = rp_mixed_formats(ctx, blobs, blobs_len, blob_off, first_flagged);
  if (rc) { memset(values, 0xFF, vals_bytes); return rc; }
  return BPMI_OK;
}
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

#include "rp_prove_host.hpp"
