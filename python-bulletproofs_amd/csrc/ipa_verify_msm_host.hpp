// ipa_verify_msm_host.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).  HOST code.
// The ending every inner-product verifier shares: ONE MSM over [g[:n] | h[:n] | extra pairs] with the s-vectors SA, SB as the
// generators' scalars, and the on-curve verdict of the device arrays read behind it.  bpmi_ipa_verify_dev, the batch calls
// (ipa_batch_host.hpp, ipa_mixed_host.hpp) and the packed ones (ipa_packed_dev_host.hpp, ipa_packed_mixed_dev_host.hpp) end here;
// the group calls (ipa_group_dev_host.hpp, ipa_group_mixed_dev_host.hpp, rp_batch_dev_host.hpp) share the pieces at the end.
#pragma once

// both plans' msm_pairs is this total (ipa_batch_plan: 2 n + n_extra; ipa_mixed_plan: 2 n_top + n_extra)
static Segs ipa_segs(const void *d_g, const void *d_h, uint64_t n, const void *sa, const void *sb, const void *d_expt, const void *d_exsc, uint64_t n_extra) {
  Segs s = segs_init();
  s.pts[0] = (const u32 *)d_g; s.sc[0] = (const u32 *)sa; s.n[0] = (u32)n;
  s.pts[1] = (const u32 *)d_h; s.sc[1] = (const u32 *)sb; s.n[1] = (u32)n;
  s.pts[2] = (const u32 *)d_expt; s.sc[2] = (const u32 *)d_exsc; s.n[2] = (u32)n_extra;
  s.total = (u32)(2 * n + n_extra);
  return s;
}

// The generators are checked from level 2, the extra points where the caller has not checked them already (queue_extra); array t of
// the verdict word is the t-th queued, so the order stands.  A failure of fetch() or msm_run leaves `out` alone; a refused call
// leaves 0xFF.. there, never the identity, which a verifier reads as "valid".
// wait_stream: hipStreamSynchronize between msm_run and the verdict.  The two packed calls wait, bpmi_ipa_verify_dev,
// bpmi_ipa_verify_batch_dev and bpmi_ipa_verify_batch_mixed_dev do not, as each did before; the verdict needs no wait beyond
// msm_run's own (DESIGN.md 6p has the reasoning and what either single form cost).
static int ipa_verify_msm(bpmi_ctx *ctx, PointCheck &pc, const void *d_g, const void *d_h, uint64_t n, const void *sa, const void *sb, const void *d_expt,
                          const void *d_exsc, uint64_t n_extra, bool queue_extra, bool wait_stream, uint8_t out[64]) {
  const Segs s = ipa_segs(d_g, d_h, n, sa, sb, d_expt, d_exsc, n_extra);
  if (ctx->opt_validate >= 2) { pc.queue(d_g, n, "d_g"); pc.queue(d_h, n, "d_h"); }
  if (queue_extra) pc.queue(d_expt, n_extra, "extra_pts");
  int rc = pc.fetch();
  if (rc) return rc;
  rc = msm_run(ctx, s, out);                    // one MSM over the three segments, sliced as any large MSM is (msm_host.hpp)
  if (rc) return rc;
  if (wait_stream) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  rc = pc.verdict();
  if (rc) memset(out, 0xFF, 64);
  return rc;
}

// ---- The pieces the GROUP calls share (bpmi_rp_batch_group_values_dev, bpmi_ipa_group_values_packed_dev and its _mixed_ twin).
// Each caller keeps its own order of launches, copies and waits; these are the lines they have in common.
// One launch of a group kernel over (group, window) on the ctx stream in the block shape the route names: `light` and `mid` are the
// kernel's <GROUP_LIGHT_THREADS, GROUP_LIGHT_NMAX> and <MID_THREADS, MID_NMAX> instantiations, J its argument struct.
template <typename J> static void group_msm_launch(bpmi_ctx *ctx, bool is_light, void (*light)(J), void (*mid)(J), u32 ngroups, u32 W, const J &job) {
  if (is_light) hipLaunchKernelGGL(light, dim3(ngroups * W), dim3(GROUP_LIGHT_THREADS), 0, ctx->stream, job);
  else hipLaunchKernelGGL(mid, dim3(ngroups * W), dim3(MID_THREADS), 0, ctx->stream, job);
}
// the device tail: the groups' window sums E[t][w] (W windows of MID_C bits) to one 64-byte value each
static void group_tail_launch(bpmi_ctx *ctx, const u32 *E, u32 W, u32 ngroups, u32 *d_vals) {
  hipLaunchKernelGGL(k_group_tail, dim3((ngroups + 63) / 64), dim3(64), 0, ctx->stream, E, W, (u32)MID_C, ngroups, d_vals);
}
// A group beyond the one-launch kernel's capacity: one MSM over [g[:n] | h[:n] | its extra pairs].  row: the scalar offset of the
// group's rows in gsa / gsb; [x0, x0 + xn): its extra pairs -- the four numbers of a row of the mixed plan's group table.
static int ipag_msm_run_group(bpmi_ctx *ctx, const void *d_g, const void *d_h, const u32 *gsa, const u32 *gsb, const u32 *x_pts, const u32 *x_sc, uint64_t n,
                              uint64_t row, uint64_t x0, uint64_t xn, uint8_t *out) {
  return msm_run(ctx, ipa_segs(d_g, d_h, n, gsa + 8 * row, gsb + 8 * row, x_pts + 16 * x0, x_sc + 8 * x0, xn), out);
}
// the end of an inner-product group call: wait, read the on-curve verdict; a refused call leaves 0xFF.. in `values`
static int ipag_finish(bpmi_ctx *ctx, PointCheck &pc, hipStream_t st, uint8_t *values, size_t vals_bytes) {
  HIPCHK(ctx, hipStreamSynchronize(st));
  const int rc = pc.verdict();
  if (rc) memset(values, 0xFF, vals_bytes);
  return rc;
}
