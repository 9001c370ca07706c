// msm_batch_host.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).
// The batched MSM: n_vec scalar vectors over one shared point set, n_vec points (bpmi_msm_batch, bpmi_msm_batch_dev,
// bpmi_msm_batch_dev_enqueue).  The plan is msm_batch_plan_host.hpp's; per row range two plain launches on the ctx stream -- k_msm_batch
// over (vector, window, part) and k_msm_batch_tail at one lane per vector (msm_kernels.hpp) --, no graph capture; the LOOP route is one
// msm_run per vector on the row's segments.  Workspace: lane 0's, so a pending asynchronous MSM that lives there refuses the call.
#pragma once

static_assert(MSMB_MID_THREADS == MID_THREADS, "msm_batch_plan_host.hpp names the block shape of k_msm_mid");
#define MSMB_PIN_BYTES (1u << 20)              // results are copied to the host through at most this much page-locked memory at a time

struct MsmBatchArgs {
  Segs segs;                                   // the non-empty segments, scalars of row 0
  u32 which[3];                                // their indices in the caller's arrays (the on-curve check names them)
  u32 nsegs;
};

// what every form checks before anything is read or allocated; fills the plan and the compacted segments
static int msmb_check(bpmi_ctx *ctx, u32 nseg, const void *const *pts, const uint64_t *n, const void *const *scalars, uint64_t n_vec, const void *out, bool host_out,
                      MsmBatchPlan &pl, MsmBatchArgs &A) {
  if (nseg < 1 || nseg > 3) return fail(ctx, BPMI_E_ARG, "nseg must be 1 .. 3");
  if (!pts || !n || !scalars || !out) return fail(ctx, BPMI_E_ARG, "null argument");
  pl = msm_batch_plan(*ctx, nseg, n, n_vec, host_out);
  if (pl.err) return fail(ctx, pl.err, pl.msg);
  if (n_vec == 0) return BPMI_OK;               // (nothing is read: the callers return at once)
  A.segs = segs_init();
  A.nsegs = 0;
  for (u32 i = 0; i < nseg; i++) {
    if (!n[i]) continue;
    if (!pts[i] || !scalars[i]) return fail(ctx, BPMI_E_ARG, "null segment");
    const u32 k = A.nsegs++;
    A.segs.pts[k] = (const u32 *)pts[i]; A.segs.sc[k] = (const u32 *)scalars[i]; A.segs.n[k] = (u32)n[i];
    A.which[k] = i;
  }
  A.segs.total = (u32)pl.total;
  return BPMI_OK;
}
// lane 0's workspace (and, on the LOOP route, slot 0) must be free: slot 0 always lives there, slots 1 and 2 unless "async_lanes" gave them lanes of their own
static int msmb_check_state(bpmi_ctx *ctx) {
  for (int s = 0; s < BPMI_LANES; s++) {
    const bool lane0 = s == 0 || !ctx->opt_async_lanes;
    if (lane0 && (ctx->pend[s].active || ctx->pend[s].async)) return fail(ctx, BPMI_E_STATE, "an MSM is still pending in a slot whose workspace this call needs (bpmi_msm_finish it first)");
  }
  return BPMI_OK;
}

// the launches of every row range; the results go to d_out (n_vec x 16 words of device memory)
static int msmb_queue(bpmi_ctx *ctx, const MsmBatchPlan &pl, const MsmBatchArgs &A, u32 *d_E, u32 *d_out) {
  BatchMsm J;
  for (int k = 0; k < 3; k++) { J.pts[k] = A.segs.pts[k]; J.sc[k] = A.segs.sc[k]; J.n[k] = A.segs.n[k]; }
  J.W = pl.W; J.parts = pl.parts; J.E = d_E;
  for (u32 k = 0; k < pl.launches; k++) {
    uint64_t v0;
    u32 cnt;
    msmb_range(pl, k, v0, cnt);
    J.v0 = (u32)v0;
    const dim3 grid(cnt * pl.W, 1, pl.parts);
    {
      StageTimer t(ctx, ST_ACCUM);
      if (pl.route == MSMB_ROUTE_LIGHT) hipLaunchKernelGGL((k_msm_batch<GROUP_LIGHT_THREADS, GROUP_LIGHT_NMAX>), grid, dim3(GROUP_LIGHT_THREADS), 0, ctx->stream, J);
      else hipLaunchKernelGGL((k_msm_batch<MID_THREADS, MID_NMAX>), grid, dim3(MID_THREADS), 0, ctx->stream, J);
    }
    {
      StageTimer t(ctx, ST_TAIL);
      hipLaunchKernelGGL(k_msm_batch_tail, dim3((cnt + 63) / 64), dim3(64), 0, ctx->stream, (const u32 *)d_E, pl.W, (u32)MID_C, pl.parts, cnt, d_out + 16 * v0);
    }
  }
  if (hipGetLastError() != hipSuccess) return fail(ctx, BPMI_E_HIP, "launch of the batched MSM failed");
  return BPMI_OK;
}
// the LOOP route: one MSM per vector, results to HOST memory
static int msmb_loop(bpmi_ctx *ctx, const MsmBatchArgs &A, uint64_t n_vec, uint8_t *out) {
  int rc = BPMI_OK;
  for (uint64_t v = 0; v < n_vec && !rc; v++) {
    Segs s = A.segs;
    for (int k = 0; k < 3; k++) s.sc[k] = A.segs.sc[k] + 8ull * A.segs.n[k] * v;
    rc = msm_run(ctx, s, out + 64 * v);
  }
  return rc;
}
// the whole batch with the results in host memory, complete on return
static int msmb_run_host(bpmi_ctx *ctx, const MsmBatchPlan &pl, const MsmBatchArgs &A, uint8_t *out) {
  const size_t bytes = 64 * (size_t)pl.n_vec;
  if (pl.route == MSMB_ROUTE_NONE) { memset(out, 0, bytes); return BPMI_OK; }
  if (pl.route == MSMB_ROUTE_LOOP) return msmb_loop(ctx, A, pl.n_vec, out);
  int rc = ensure_ws(ctx, pl.total_bytes, 0);
  if (rc == BPMI_OK) rc = ensure_pin(ctx, std::min<size_t>(bytes, MSMB_PIN_BYTES));
  if (rc) return rc;
  char *ws = (char *)ctx->lane[0].ws;
  rc = msmb_queue(ctx, pl, A, (u32 *)(ws + pl.o_E), (u32 *)(ws + pl.o_out));
  if (rc) return rc;
  for (size_t off = 0; off < bytes; off += MSMB_PIN_BYTES) {
    const size_t len = std::min<size_t>(bytes - off, MSMB_PIN_BYTES);
    HIPCHK(ctx, hipMemcpyAsync(ctx->pin, ws + pl.o_out + off, len, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, wait_stream(ctx, ctx->stream));
    memcpy(out + off, ctx->pin, len);
  }
  return BPMI_OK;
}

extern "C" {

int bpmi_msm_batch_dev(bpmi_ctx *ctx, uint32_t nseg, const void *const *d_pts, const uint64_t *n, const void *const *d_scalars, uint64_t n_vec, uint8_t *out) {
  if (!ctx) return BPMI_E_ARG;
  MsmBatchPlan pl;
  MsmBatchArgs A;
  int rc = msmb_check(ctx, nseg, d_pts, n, d_scalars, n_vec, out, true, pl, A);
  if (rc || n_vec == 0) return rc;
  if ((rc = msmb_check_state(ctx))) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  static const char *const names[3] = {"d_pts[0]", "d_pts[1]", "d_pts[2]"};      // by the caller's segment number, A.which
  PointCheck pc(ctx, "bpmi_msm_batch_dev", ctx->stream, ctx->opt_validate >= 2);
  for (u32 k = 0; k < A.nsegs; k++) pc.queue(A.segs.pts[k], A.segs.n[k], names[A.which[k]]);
  rc = pc.fetch();
  if (rc) return rc;
  rc = msmb_run_host(ctx, pl, A, out);
  if (rc) return rc;
  rc = pc.verdict();
  if (rc) memset(out, 0, 64 * (size_t)n_vec);
  return rc;
}

int bpmi_msm_batch_dev_enqueue(bpmi_ctx *ctx, uint32_t nseg, const void *const *d_pts, const uint64_t *n, const void *const *d_scalars, uint64_t n_vec, void *d_out) {
  if (!ctx) return BPMI_E_ARG;
  MsmBatchPlan pl;
  MsmBatchArgs A;
  int rc = msmb_check(ctx, nseg, d_pts, n, d_scalars, n_vec, d_out, false, pl, A);
  if (rc || n_vec == 0) return rc;
  if ((rc = msmb_check_state(ctx))) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t bytes = 64 * (size_t)n_vec;
  if (pl.route == MSMB_ROUTE_NONE) { HIPCHK(ctx, hipMemsetAsync(d_out, 0, bytes, ctx->stream)); return BPMI_OK; }
  if (pl.route == MSMB_ROUTE_LOOP) {
    // (the loop's MSMs finish on the host: this route waits, and hands the results over through the stream)
    std::vector<uint8_t> tmp(bytes);
    if ((rc = msmb_loop(ctx, A, n_vec, tmp.data()))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(d_out, tmp.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return BPMI_OK;
  }
  if ((rc = ensure_ws(ctx, pl.total_bytes, 0))) return rc;
  return msmb_queue(ctx, pl, A, (u32 *)((char *)ctx->lane[0].ws + pl.o_E), (u32 *)d_out);
}

int bpmi_msm_batch(bpmi_ctx *ctx, const uint8_t *pts, uint64_t n, const uint8_t *scalars, uint64_t n_vec, uint8_t *out) {
  if (!ctx) return BPMI_E_ARG;
  if (!out || (n && (!pts || !scalars))) return fail(ctx, BPMI_E_ARG, "null argument");
  const uint64_t ns[1] = {n};
  {
    const MsmBatchPlan pre = msm_batch_plan(*ctx, 1, ns, n_vec, true);
    if (pre.err) return fail(ctx, pre.err, pre.msg);
  }
  if (n_vec == 0) return BPMI_OK;
  if (n == 0) { memset(out, 0, 64 * (size_t)n_vec); return BPMI_OK; }
  int rc = msmb_check_state(ctx);
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t o_sc = align_up(64 * n, 256), sc_bytes = 32 * (size_t)n * (size_t)n_vec;
  rc = ensure_stage_in(ctx, o_sc + sc_bytes + 512);
  if (rc) return rc;
  char *dp = (char *)ctx->stage_in, *ds = dp + o_sc;
  HIPCHK(ctx, h2d(ctx, dp, pts, 64 * n, ctx->stream));
  HIPCHK(ctx, h2d(ctx, ds, scalars, sc_bytes, ctx->stream));
  PointCheck pc(ctx, "bpmi_msm_batch", ctx->stream, ctx->opt_validate >= 1);
  pc.queue(dp, n, "pts");
  rc = pc.fetch();
  if (rc) return rc;
  const void *const P[1] = {dp}, *const S[1] = {ds};
  MsmBatchPlan pl;
  MsmBatchArgs A;
  rc = msmb_check(ctx, 1, P, ns, S, n_vec, out, true, pl, A);
  if (rc == BPMI_OK) rc = msmb_run_host(ctx, pl, A, out);
  if (rc) return rc;
  rc = pc.verdict();
  if (rc) memset(out, 0, 64 * (size_t)n_vec);
  return rc;
}

}  // extern "C"
