// msm_fixed_host.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).
// Host side of the fixed-base MSM: the object that owns a point set and the table of its multiples (msm_fixed_plan_host.hpp), the build
// of that table (k_fixed_table_row) and the one way an MSM over it reaches msm_enqueue.  The entry points are in bpmi.hip.
#pragma once
#include <chrono>

struct bpmi_fixed_base {
  bpmi_ctx *ctx = nullptr;
  FixedPlan plan;
  u32 *table = nullptr;          // plan.R rows of plan.n affine points, row-major: virtual pair r n + i
  double build_us = 0;           // copy of the points, their check and the rows, until the stream ran dry
};
// one MSM over the object's points: the first n_scalars of them
struct FixedBaseCall { const bpmi_fixed_base *fx; const void *d_scalars; uint64_t n_scalars; };

// Queue the MSM of `call` into pending slot `slot` on `lane`, exactly as msm_enqueue queues an ordinary one (it IS msm_enqueue: the slot's
// BPMI_E_STATE rule, the workspace and the pinned buffer are its own).  R = 1: the ordinary MSM over the copy of the points, with the
// object's window bits forced for the length of the call (none: the automatic rule left the choice to the ctx's options).
static int fixed_base_enqueue(bpmi_ctx *ctx, const MsmMode &mode, int lane, int slot, const FixedBaseCall &call) {
  const bpmi_fixed_base &fx = *call.fx;
  const FixedPlan &p = fx.plan;
  Segs s = segs_init();
  s.pts[0] = fx.table; s.sc[0] = (const u32 *)call.d_scalars;
  if (p.R == 1u) {
    s.n[0] = s.total = (u32)call.n_scalars;
    const int keep = ctx->opt_c;
    if (p.c) ctx->opt_c = (int)p.c;
    const int rc = msm_enqueue(ctx, mode, lane, slot, s);
    ctx->opt_c = keep;
    return rc;
  }
  s.n[0] = s.total = call.n_scalars ? (u32)(p.n * p.R) : 0u;        // (no scalars: msm_enqueue leaves the slot empty, the identity)
  MsmRecode rec;
  rec.plan = fixed_virtual_geometry(*ctx, mode, p);
  rec.sc = segs_init();
  rec.sc.sc[0] = (const u32 *)call.d_scalars; rec.sc.n[0] = rec.sc.total = (u32)call.n_scalars;
  rec.real = fixed_real_geometry(p);
  rec.n_scalars = (u32)call.n_scalars; rec.R = p.R; rec.Wv = p.Wv;
  return msm_enqueue(ctx, mode, lane, slot, s, 0, 0, 0, &rec);
}
// the synchronous MSM: slot 0 on lane 0, as msm_run's
static int fixed_base_run(bpmi_ctx *ctx, const FixedBaseCall &call, uint8_t out[64]) {
  if (call.fx->plan.R == 1u && !call.fx->plan.c) {                   // today's MSM, slices and all
    Segs s = segs_init();
    s.pts[0] = call.fx->table; s.sc[0] = (const u32 *)call.d_scalars; s.n[0] = s.total = (u32)call.n_scalars;
    return msm_run(ctx, s, out);
  }
  const int rc = fixed_base_enqueue(ctx, MsmMode{}, 0, 0, call);
  if (rc) return rc;
  return msm_finish(ctx, 0, out);
}

// Build the object over the n points at d_pts (device memory; copied).  check: the points are checked to be on the curve.
static int fixed_base_build(bpmi_ctx *ctx, const char *fn, const void *d_pts, const FixedPlan &p, bool check, bpmi_fixed_base **out) {
  const auto t0 = std::chrono::steady_clock::now();
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  u32 *table = nullptr, *scratch = nullptr;
  HIPCHK(ctx, hipMalloc((void **)&table, (size_t)p.table_bytes));
  auto work = [&]() -> int {
    if (p.R > 1u) HIPCHK(ctx, hipMalloc((void **)&scratch, fixed_table_scratch_bytes(p.n)));
    HIPCHK(ctx, hipMemcpyAsync(table, d_pts, 64ull * p.n, hipMemcpyDeviceToDevice, st));
    PointCheck pc(ctx, fn, st, check);
    pc.queue(table, p.n, "pts");
    int rc = pc.fetch();
    if (rc) return rc;
    const u32 ncols = (u32)((p.n + FIXED_TAB_PER - 1u) / FIXED_TAB_PER);
    for (u32 r = 1; r < p.R; r++)
      hipLaunchKernelGGL(k_fixed_table_row, dim3((ncols + 255u) / 256u), dim3(256), 0, st, table + 16ull * p.n * (r - 1u), table + 16ull * p.n * r, (u32)p.n,
                         p.c * p.Wv, scratch);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st));
    return pc.verdict();
  };
  const int rc = work();
  if (rc) (void)hipStreamSynchronize(st);
  if (scratch) (void)hipFree(scratch);
  if (rc) { (void)hipFree(table); return rc; }
  bpmi_fixed_base *fx = new bpmi_fixed_base();
  fx->ctx = ctx; fx->plan = p; fx->table = table;
  fx->build_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  *out = fx;
  return BPMI_OK;
}
