// ipa_group_mixed_dev_host.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).  HOST code.
// Which groups of a list of classes of PACKED inner-product proofs of DIFFERENT lengths hold an invalid one:
// bpmi_ipa_group_values_packed_mixed_dev.  The preparation of bpmi_ipa_verify_batch_packed_mixed_dev (ipapm_run: uploads, re-hash,
// inversion, weights -- once per call) and its mixed half tables (ipam_control_upload, ipam_tables_launch, ipa_mixed_host.hpp), but
// the s-vectors are summed per GROUP of consecutive proofs of one class (k_sc_svector_sum_groups_mixed, one launch over every class's
// rows) and the groups' MSMs over [g[:n_c] | h[:n_c] | the group's extra pairs] run as at most one launch per block shape over
// (group, window) (k_msm_ipa_group_mixed) with ONE device tail (k_group_tail); the groups of a class beyond the kernel's capacity go
// through msm_run one by one.  The counterpart of bpmi_ipa_group_values_packed_dev (ipa_group_dev_host.hpp) for a list of classes:
// its own preparation, sum launch and order of copies and waits here, the shared pieces in ipa_verify_msm_host.hpp.
// Plan, argument errors and routes: ipa_group_mixed_plan_host.hpp.
#pragma once

extern "C" {

int bpmi_ipa_group_values_packed_mixed_dev(bpmi_ctx *ctx, const void *d_g, const void *d_h, const void *d_hscale, uint64_t n_gens, int protocol, uint32_t n_classes,
                                           const bpmi_ipa_packed_class *classes, const uint64_t *group, const uint8_t *weights, const uint8_t *seed, uint8_t *values,
                                           uint64_t *value_off, uint8_t *status) {
  static const char *const fn = "bpmi_ipa_group_values_packed_mixed_dev";
  if (!ctx) return BPMI_E_ARG;
  u32 K;
  if (!log2_exact(n_gens, K) || K > IPAB_K_MAX) return fail(ctx, BPMI_E_ARG, std::string(fn) + ": n_gens must be 2^K, K <= 22");
  const IpagmPlan gp = ipa_group_mixed_plan(*ctx, K, protocol, n_classes, classes, group, weights, seed, d_hscale ? 1 : 0, values && value_off && status, ctx->ipap_t_budget);
  if (gp.err) return fail(ctx, gp.err, std::string(fn) + ": " + gp.msg);
  if (!gp.empty && (!d_g || !d_h)) return fail(ctx, BPMI_E_ARG, std::string(fn) + ": null argument");
  for (u32 c = 0; c <= n_classes; c++) value_off[c] = gp.value_off[c];
  if (gp.empty) return BPMI_OK;
  const IpapmPlan &mp = gp.packed;
  const IpamPlan &bp = mp.base;
  const size_t vals_bytes = 64 * (size_t)gp.ngroups;
  // the proofs' points are the preparation's to check (status bit 1); the classes' u of Protocol 1 here, the first n_top generators at
  // level 2 by a kernel whose verdict is read after the call's synchronisation; a refused call leaves 0xFF.. in `values`
  PointCheck pc(ctx, fn, ctx->stream, ctx->opt_validate >= 1);
  int rc = ipapm_check_us(pc, mp, classes);
  if (rc) { memset(values, 0xFF, vals_bytes); return rc; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  rc = ensure_stage_in(ctx, gp.total_bytes + 512);
  if (rc) return rc;
  char *base = (char *)ctx->stage_in;
  hipStream_t st = ctx->stream;
  std::vector<uint8_t> tables;                                 // (lives until the stream has been waited for: ipam_control_upload waits)
  rc = ipapm_run(ctx, mp, classes, weights, seed, (u32 *)(base + bp.o_rec), (u32 *)(base + bp.o_expt), (u32 *)(base + bp.o_exsc), tables);
  if (rc) { (void)hipStreamSynchronize(st); return rc; }
  HIPCHK(ctx, hipMemcpyAsync(status, base + mp.o_status, mp.b_status, hipMemcpyDeviceToHost, st));
  // the class table, the group table and the two lists: one piece, owned by this frame until the wait of ipam_control_upload
  std::vector<uint8_t> gtabs(gp.total_bytes - gp.o_ctab, 0);
  memcpy(gtabs.data(), gp.class_tab.data(), gp.b_ctab);
  memcpy(gtabs.data() + (gp.o_gtab - gp.o_ctab), gp.group_tab.data(), gp.b_gtab);
  if (gp.b_light) memcpy(gtabs.data() + (gp.o_light - gp.o_ctab), gp.light.data(), gp.b_light);
  if (gp.b_mid) memcpy(gtabs.data() + (gp.o_mid - gp.o_ctab), gp.mid.data(), gp.b_mid);
  HIPCHK(ctx, h2d(ctx, base + gp.o_ctab, gtabs.data(), gtabs.size(), st));
  rc = ipam_control_upload(ctx, bp);
  if (rc) { (void)hipStreamSynchronize(st); return rc; }
  u32 *gsa = (u32 *)(base + gp.o_gsa), *gsb = (u32 *)(base + gp.o_gsb);
  {
    StageTimer t(ctx, ST_SCFOLD);
    ipam_tables_launch(ctx, bp);
    hipLaunchKernelGGL(k_sc_svector_sum_groups_mixed, dim3(gp.n_blocks), dim3(IPAGM_BLOCK), 0, st, (const u32 *)(base + bp.o_tab), (const u32 *)(base + gp.o_ctab),
                       (u32)(gp.class_tab.size() / IPAGM_CLASS_WORDS), (const u32 *)d_hscale, gsa, gsb);
  }
  HIPCHK(ctx, hipGetLastError());
  if (ctx->opt_validate >= 2) { pc.queue(d_g, bp.n_top, "d_g"); pc.queue(d_h, bp.n_top, "d_h"); }
  rc = pc.fetch();
  if (rc) return rc;
  u32 *d_E = (u32 *)(base + gp.o_E), *d_vals = (u32 *)(base + gp.o_vals);
  const u32 *x_pts = (const u32 *)(base + bp.o_expt), *x_sc = (const u32 *)(base + bp.o_exsc);
  {
    IpaGroupMixedMsm J;
    J.g = (const u32 *)d_g; J.h = (const u32 *)d_h; J.sa = gsa; J.sb = gsb; J.x_pts = x_pts; J.x_sc = x_sc;
    J.gtab = (const u32 *)(base + gp.o_gtab); J.W = gp.W; J.E = d_E;
    StageTimer t(ctx, ST_ACCUM);
    // the groups that msm_run takes leave no window sums: theirs are the identity for the tail, and msm_run writes their values below
    if (!gp.run.empty()) HIPCHK(ctx, hipMemsetAsync(d_E, 0, gp.b_E, st));
    for (const bool is_light : {true, false}) {                  // at most one launch per block shape, over that shape's list
      const std::vector<u32> &list = is_light ? gp.light : gp.mid;
      if (list.empty()) continue;
      J.list = (const u32 *)(base + (is_light ? gp.o_light : gp.o_mid));
      group_msm_launch(ctx, is_light, k_msm_ipa_group_mixed<GROUP_LIGHT_THREADS, GROUP_LIGHT_NMAX>, k_msm_ipa_group_mixed<MID_THREADS, MID_NMAX>, (u32)list.size(), gp.W, J);
    }
    group_tail_launch(ctx, d_E, gp.W, gp.ngroups, d_vals);
  }
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(values, d_vals, vals_bytes, hipMemcpyDeviceToHost, st));
  if (!gp.run.empty()) {
    // groups beyond the one-launch kernel's capacity, behind the copy and a wait of this call's own (the uniform call has neither)
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (const u32 t : gp.run) {
      const u32 *d = gp.group_tab.data() + (size_t)IPAGM_GROUP_WORDS * t;          // n_c, row offset, first extra pair, extra pairs
      rc = ipag_msm_run_group(ctx, d_g, d_h, gsa, gsb, x_pts, x_sc, d[0], d[1], d[2], d[3], values + 64 * (size_t)t);
      if (rc) { memset(values, 0xFF, vals_bytes); return rc; }
    }
  }
  return ipag_finish(ctx, pc, st, values, vals_bytes);
}

}  // extern "C"
