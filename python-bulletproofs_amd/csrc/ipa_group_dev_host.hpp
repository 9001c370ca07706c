// ipa_group_dev_host.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).  HOST code.
// Which groups of a batch of PACKED inner-product proofs hold an invalid one: bpmi_ipa_group_values_packed_dev.  The preparation of
// bpmi_ipa_verify_batch_packed_dev (ipap_run: upload, re-hash, inversion, weights -- once per batch) and its half tables
// (ipab_tables_launch, ipa_batch_host.hpp), but the s-vectors are summed per GROUP of `group` consecutive proofs
// (k_sc_svector_sum_groups) and the groups' MSMs over [g | h | the group's extra pairs] run as ONE launch over (group, window)
// (k_msm_ipa_group) with a device tail (k_group_tail) -- the counterpart of bpmi_rp_batch_group_values_dev.  This file holds the
// call's preparation, its sum launch and its order of copies and waits; the launch lines, the msm_run of one group and the ending
// are the group calls' shared pieces (ipa_verify_msm_host.hpp).  Plan, argument errors and routes: ipa_group_plan_host.hpp.
#pragma once

extern "C" {

int bpmi_ipa_group_values_packed_dev(bpmi_ctx *ctx, const void *d_g, const void *d_h, const void *d_hscale, uint64_t n, int protocol, uint64_t n_proofs,
                                     const uint8_t *ab, const uint8_t *xs, const uint8_t *LR, const uint8_t *transcripts, const uint64_t *tr_off,
                                     const uint32_t *start, const uint8_t *u, const uint8_t *P, const uint8_t *c, const uint8_t *head, const uint8_t *weights,
                                     const uint8_t *seed, uint64_t group, uint8_t *values, uint8_t *status) {
  static const char *const fn = "bpmi_ipa_group_values_packed_dev";
  if (!ctx) return BPMI_E_ARG;
  if (n_proofs == 0) return BPMI_OK;
  if (!d_g || !d_h) return fail(ctx, BPMI_E_ARG, std::string(fn) + ": null argument");
  const IpaPackedIn in = ipap_in(ab, xs, LR, transcripts, tr_off, start, u, P, c, head, weights, seed);
  const IpagPlan gp = ipa_group_plan(*ctx, n, protocol, n_proofs, in, d_hscale ? 1 : 0, group, values && status, ctx->ipap_t_budget);
  if (gp.err) return fail(ctx, gp.err, std::string(fn) + ": " + gp.msg);
  const IpapPlan &pl = gp.packed;
  const IpabPlan &bp = pl.base;
  const size_t vals_bytes = 64 * (size_t)gp.ngroups;
  // the proofs' points are the preparation's to check (status bit 1); the shared u of Protocol 1 here, the generators at level 2 by a
  // kernel whose verdict is read after the call's synchronisation; a refused call leaves 0xFF.. in `values`
  PointCheck pc(ctx, fn, ctx->stream, ctx->opt_validate >= 1);
  int rc = protocol == 1 ? pc.host(u, 1, "u") : BPMI_OK;
  if (rc) { memset(values, 0xFF, vals_bytes); return rc; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  rc = ensure_stage_in(ctx, gp.total_bytes + 512);
  if (rc) return rc;
  char *base = (char *)ctx->stage_in;
  hipStream_t st = ctx->stream;
  rc = ipap_run(ctx, pl, in, (u32 *)(base + bp.o_rec), (u32 *)(base + bp.o_expt), (u32 *)(base + bp.o_exsc));
  if (rc) return rc;
  HIPCHK(ctx, hipMemcpyAsync(status, base + pl.o_status, n_proofs, hipMemcpyDeviceToHost, st));
  const u32 nn = (u32)n, Pn = (u32)n_proofs, ntab = (u32)bp.tab_entries;
  u32 *gsa = (u32 *)(base + gp.o_gsa), *gsb = (u32 *)(base + gp.o_gsb);
  {
    StageTimer t(ctx, ST_SCFOLD);
    ipab_tables_launch(ctx, bp);
    const uint64_t elems = (uint64_t)gp.ngroups * n;                   // <= 2^25 (the plan's cap)
    hipLaunchKernelGGL(k_sc_svector_sum_groups, dim3((u32)((elems + 255) / 256)), dim3(256), 0, st, (const u32 *)(base + bp.o_tab), ntab, bp.k, bp.kl, Pn,
                       gp.group, gp.ngroups, (const u32 *)d_hscale, gsa, gsb);
  }
  HIPCHK(ctx, hipGetLastError());
  if (ctx->opt_validate >= 2) { pc.queue(d_g, n, "d_g"); pc.queue(d_h, n, "d_h"); }
  rc = pc.fetch();
  if (rc) return rc;
  const u32 *x_pts = (const u32 *)(base + bp.o_expt), *x_sc = (const u32 *)(base + bp.o_exsc);
  if (gp.route != IPAG_ROUTE_MSM_RUN) {
    IpaGroupMsm J;
    J.g = (const u32 *)d_g; J.h = (const u32 *)d_h; J.sa = gsa; J.sb = gsb; J.x_pts = x_pts; J.x_sc = x_sc;
    J.n = nn; J.per = gp.per; J.group = gp.group; J.P = Pn; J.W = gp.W; J.E = (u32 *)(base + gp.o_E);
    u32 *d_vals = (u32 *)(base + gp.o_vals);
    {
      StageTimer t(ctx, ST_ACCUM);
      group_msm_launch(ctx, gp.route == IPAG_ROUTE_LIGHT, k_msm_ipa_group<GROUP_LIGHT_THREADS, GROUP_LIGHT_NMAX>, k_msm_ipa_group<MID_THREADS, MID_NMAX>, gp.ngroups, gp.W, J);
      group_tail_launch(ctx, J.E, gp.W, gp.ngroups, d_vals);
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(values, d_vals, vals_bytes, hipMemcpyDeviceToHost, st));
  } else {
    // no values copy and no wait in front of the loop on this route: msm_run writes `values` itself (as rp_run_group_msms)
    for (u32 t = 0; t < gp.ngroups; t++) {
      const uint64_t g0 = (uint64_t)t * gp.group, cnt = std::min<uint64_t>(gp.group, n_proofs - g0);
      rc = ipag_msm_run_group(ctx, d_g, d_h, gsa, gsb, x_pts, x_sc, n, n * t, gp.per * g0, cnt * gp.per, values + 64 * (size_t)t);
      if (rc) { memset(values, 0xFF, vals_bytes); return rc; }
    }
  }
  return ipag_finish(ctx, pc, st, values, vals_bytes);
}

}  // extern "C"
