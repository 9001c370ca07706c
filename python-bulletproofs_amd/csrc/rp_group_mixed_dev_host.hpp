// rp_group_mixed_dev_host.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).  HOST code.
// Which groups of a MIXED batch of range proofs hold an invalid one: bpmi_rp_batch_group_values_mixed_dev.  It is rp_mixed_enqueue
// (rp_mixed_dev_host.hpp) with group mode on -- every class's uploads, word-major proofs and point decoding in its own regions, per ROUND
// one launch of each chain kernel over all classes (k_rp_roles_mixed, k_rp_elements_mixed), then per unit the verdict bytes and the
// per-group column sums of that class's chunk (rp_queue_group_rows of rp_batch_dev_host.hpp, as it is) and per class k_rp_group_scalars --
// followed here by the generator copies, at most one k_msm_group_mixed launch per block shape over (group, window), ONE device tail
// (k_group_tail) over all groups, one copy of the values and one of the verdict bytes of all classes.  The groups of a class beyond the
// one-launch kernel's capacity go through msm_run one by one, as rp_run_group_msms does for a batch of one size.
// What the mixed verify call has and this path does not need: k_rp_shared_scalars / k_rp_shared_merge are not launched (the merged region
// stays laid out, unused), and the call's one bad word is laid out and WRITTEN (the roles and the decoder report into it) but never
// read -- the verdict bytes say more.
// Plan, argument errors and routes: rp_group_mixed_plan_host.hpp.
#pragma once

static_assert(RPGM_GENS_DIRECT == GroupMixedMsm::GENS_DIRECT && RPGM_GROUP_WORDS == 8u, "k_msm_group_mixed reads the plan's group table");

// the contiguous copies [g h u gs[:n] hs[:n]] of the prefixes shorter than the list: three device-to-device copies each
static int rpgm_queue_copies(bpmi_ctx *ctx, const RpgmPlan &gp, const void *d_gens) {
  const char *src = (const char *)d_gens;
  for (const RpgmCopy &k : gp.copies) {
    char *dst = (char *)ctx->rp_buf + k.at.off;
    HIPCHK(ctx, hipMemcpyAsync(dst, src, 64 * 3, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(dst + 64 * 3, src + 64 * 3, 64 * (size_t)k.n, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(dst + 64 * (3 + (size_t)k.n), src + 64 * (3 + (size_t)gp.mixed.N), 64 * (size_t)k.n, hipMemcpyDeviceToDevice, ctx->stream));
  }
  return BPMI_OK;
}

// a group on the msm_run route: one MSM over [its generators | its commitments | its proof points]; d: its row of the group table
static int rpgm_msm_run_group(bpmi_ctx *ctx, const u32 *gens, const u32 *copies, const u32 *gfin, const void *d_points, const void *d_scalars, const u32 *d, uint8_t *out) {
  Segs s = segs_init();
  s.pts[0] = d[0] == RPGM_GENS_DIRECT ? gens : copies + 16ull * d[0]; s.sc[0] = gfin + (uint64_t)d[2]; s.n[0] = d[1];
  s.pts[1] = (const u32 *)d_points + 16ull * d[3]; s.sc[1] = (const u32 *)d_scalars + 8ull * d[3]; s.n[1] = d[4];
  s.pts[2] = (const u32 *)d_points + 16ull * d[5]; s.sc[2] = (const u32 *)d_scalars + 8ull * d[5]; s.n[2] = d[6];
  s.total = s.n[0] + s.n[1] + s.n[2];
  return msm_run(ctx, s, out);
}

extern "C" {

int bpmi_rp_batch_group_values_mixed_dev(bpmi_ctx *ctx, uint32_t n_classes, const bpmi_rp_class *classes, uint32_t n_gens_max, const uint64_t *group,
                                         const uint8_t *weights, const uint8_t *seed, const void *d_gens, void *d_points, void *d_scalars, uint8_t *values,
                                         uint64_t *value_off, uint8_t *status) {
  if (!ctx) return BPMI_E_ARG;
  const RpgmPlan gp = rp_group_mixed_plan(*ctx, n_classes, classes, n_gens_max, group, weights != nullptr, seed != nullptr, d_gens && d_points && d_scalars,
                                          values && value_off && status);
  if (gp.err) return fail(ctx, gp.err, gp.msg);
  const RpMixedPlan &mp = gp.mixed;
  for (u32 c = 0; c <= n_classes; c++) value_off[c] = gp.value_off[c];
  const size_t vals_bytes = 64 * (size_t)gp.ngroups;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  PointCheck pc(ctx, "bpmi_rp_batch_group_values_mixed_dev", ctx->stream, ctx->opt_validate >= 1);
  std::vector<uint8_t> table, gtabs;                           // (both live until the lanes have been waited for)
  std::vector<RpGroups> groups;
  u32 *d_merged = nullptr;
  unsigned long long *d_bad = nullptr;
  int rc = rp_mixed_enqueue(ctx, mp, classes, weights, seed, d_points, d_scalars, pc, d_gens, table, d_merged, d_bad, &gp, &groups);
  // an error in the middle must not return while the second lane is still writing into the caller's point array
  if (rc) { memset(values, 0xFF, vals_bytes); return rp_wait_lanes(ctx, rc); }
  char *buf = (char *)ctx->rp_buf;
  rc = rpgm_queue_copies(ctx, gp, d_gens);
  if (!rc) {
    // the group table and the two lists: one piece
    gtabs.assign(gp.mid_list.off + gp.mid_list.bytes - gp.gtab.off, 0);
    memcpy(gtabs.data(), gp.group_tab.data(), gp.gtab.bytes);
    if (gp.light_list.bytes) memcpy(gtabs.data() + (gp.light_list.off - gp.gtab.off), gp.light.data(), gp.light_list.bytes);
    if (gp.mid_list.bytes) memcpy(gtabs.data() + (gp.mid_list.off - gp.gtab.off), gp.mid.data(), gp.mid_list.bytes);
    if (h2d(ctx, buf + gp.gtab.off, gtabs.data(), gtabs.size(), ctx->stream) != hipSuccess) rc = fail(ctx, BPMI_E_HIP, "upload of the group table failed");
  }
  const u32 *copies = (const u32 *)(buf + gp.copies_base), *gfin = (const u32 *)(buf + gp.gfin_base);
  u32 *d_E = (u32 *)(buf + gp.E.off), *d_vals = (u32 *)(buf + gp.vals.off);
  if (!rc) {
    GroupMixedMsm J;
    J.gens = (const u32 *)d_gens; J.copies = copies; J.gfin = gfin;
    J.pts = (const u32 *)d_points; J.sc = (const u32 *)d_scalars;
    J.gtab = (const u32 *)(buf + gp.gtab.off); J.W = gp.W; J.E = d_E;
    StageTimer t(ctx, ST_ACCUM);
    // the groups that msm_run takes leave no window sums: theirs are the identity for the tail, and msm_run writes their values below
    if (!gp.run.empty() && hipMemsetAsync(d_E, 0, gp.E.bytes, ctx->stream) != hipSuccess) rc = fail(ctx, BPMI_E_HIP, "clearing the window sums failed");
    for (const bool is_light : {true, false}) {                  // at most one launch per block shape, over that shape's list
      const std::vector<u32> &list = is_light ? gp.light : gp.mid;
      if (list.empty() || rc) continue;
      J.list = (const u32 *)(buf + (is_light ? gp.light_list.off : gp.mid_list.off));
      group_msm_launch(ctx, is_light, k_msm_group_mixed<GROUP_LIGHT_THREADS, GROUP_LIGHT_NMAX>, k_msm_group_mixed<MID_THREADS, MID_NMAX>, (u32)list.size(), gp.W, J);
    }
    if (!rc) group_tail_launch(ctx, d_E, gp.W, gp.ngroups, d_vals);
    if (!rc && hipGetLastError() != hipSuccess) rc = fail(ctx, BPMI_E_HIP, "launch of the group MSMs failed");
  }
  if (!rc && hipMemcpyAsync(ctx->pin, d_vals, vals_bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = fail(ctx, BPMI_E_HIP, "copy of the group values failed");
  if (!rc && hipMemcpyAsync((char *)ctx->pin + vals_bytes, buf + gp.verdict.off, mp.n_proofs, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
    rc = fail(ctx, BPMI_E_HIP, "copy of the verdicts failed");
  rc = rp_wait_lanes(ctx, rc);
  if (rc) { memset(values, 0xFF, vals_bytes); return rc; }
  memcpy(values, ctx->pin, vals_bytes);
  memcpy(status, (char *)ctx->pin + vals_bytes, mp.n_proofs);
  for (size_t i = 0; i < gp.run.size() && !rc; i++) {
    const u32 t = gp.run[i];
    rc = rpgm_msm_run_group(ctx, (const u32 *)d_gens, copies, gfin, d_points, d_scalars, gp.group_tab.data() + (size_t)RPGM_GROUP_WORDS * t, values + 64 * (size_t)t);
  }
  if (!gp.run.empty()) rc = rp_wait_lanes(ctx, rc);
  if (!rc) rc = pc.verdict();
  // a well-formed proof of another wire format at a class's smallest flagged index is a sender's mix-up, not a verdict
  for (u32 c = 0; c < n_classes && !rc; c++) {
    const uint8_t *st = status + mp.cls[c].first;
    int64_t first_flagged = -1;
    for (uint64_t i = 0; i < classes[c].n_proofs && first_flagged < 0; i++) if (st[i]) first_flagged = (int64_t)i;
    rc = rp_mixed_formats(ctx, classes[c].blobs, classes[c].blobs_len, classes[c].blob_off, first_flagged, (int)c);
  }
  if (rc) memset(values, 0xFF, vals_bytes);
  return rc;
}

}  // extern "C"
