// ipa_mixed_host.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).  HOST code.
// Batch verification of inner-product proofs of DIFFERENT lengths over the prefixes of one generator list: bpmi_sc_svector_sum_mixed
// and bpmi_ipa_verify_batch_mixed_dev.  The weighted equation of ipa_batch_host.hpp, with proof p of n_p = 2^k_p elements stated over
// g[:n_p], h[:n_p] (Verifier2.verify and get_ss, src/innerproduct/inner_product_verifier.py:127-147 and :91-102 of the reference, per
// proof over its prefix): generator i collects the proofs with n_p > i, so the batch is still ONE MSM, of 2 n_top + (extra pairs),
// n_top = max n_p, and the s-vector sums cost sum_p n_p x 2 multiplications.  Plan: ipa_mixed_plan_host.hpp; kernels:
// ipa_mixed_kernels.hpp.
#pragma once

extern "C" {

// the control regions -- descriptors, C table, units, block index -- uploaded as one piece and waited for
static int ipam_control_upload(bpmi_ctx *ctx, const IpamPlan &pl) {
  char *base = (char *)ctx->stage_in;
  std::vector<uint8_t> control(pl.o_tab - pl.o_desc);
  uint8_t *at = control.data();
  memcpy(at, pl.desc.data(), pl.b_desc);
  memcpy(at + (pl.o_ctab - pl.o_desc), pl.C.data(), pl.b_ctab);
  memcpy(at + (pl.o_units - pl.o_desc), pl.unit.data(), pl.b_units);
  memcpy(at + (pl.o_blocks - pl.o_desc), pl.block_first.data(), pl.b_blocks);
  HIPCHK(ctx, h2d(ctx, base + pl.o_desc, control.data(), control.size(), ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));          // control (and the caller's records) are owned by host frames
  return BPMI_OK;
}
// every proof's half tables from the records in the workspace: one launch (inside the caller's stage timer)
static void ipam_tables_launch(bpmi_ctx *ctx, const IpamPlan &pl) {
  char *base = (char *)ctx->stage_in;
  const u32 n_records = (u32)pl.tab_entries;
  hipLaunchKernelGGL(k_sc_svector_tables_mixed, dim3((n_records + IPAB_THREADS - 1) / IPAB_THREADS), dim3(IPAB_THREADS), 0, ctx->stream,
                     (const u32 *)(base + pl.o_rec), (const u32 *)(base + pl.o_desc), (u32)pl.n_proofs, n_records, (u32 *)(base + pl.o_tab));
}
// the three launches that leave SA and SB in the workspace, from the proofs' records (sorted order) that are in the workspace
// already: uploaded by ipam_svector_sum, or written there by the preparation kernels (ipa_packed_mixed_dev_host.hpp).  Only the control
// regions are uploaded here.  (The group call, ipa_group_mixed_dev_host.hpp, takes the upload and the tables alone.)
static int ipam_svector_launches(bpmi_ctx *ctx, const IpamPlan &pl, const void *d_scale) {
  char *base = (char *)ctx->stage_in;
  const int rc = ipam_control_upload(ctx, pl);
  if (rc) return rc;
  const u32 *desc = (const u32 *)(base + pl.o_desc), *tabs = (const u32 *)(base + pl.o_tab);
  u32 *sa = (u32 *)(base + pl.o_sa), *sb = (u32 *)(base + pl.o_sb), *part = (u32 *)(base + pl.o_part);
  const u32 n_top = (u32)pl.n_top;
  {
    StageTimer t(ctx, ST_SCFOLD);
    ipam_tables_launch(ctx, pl);
    hipLaunchKernelGGL(k_sc_svector_sum_mixed, dim3(pl.n_units), dim3(IPAB_THREADS), 0, ctx->stream, tabs, desc, (const u32 *)(base + pl.o_ctab),
                       (const u32 *)(base + pl.o_units), n_top, pl.direct ? 1u : 0u, pl.direct ? sa : part, pl.direct ? sb : part);
    if (!pl.direct)
      hipLaunchKernelGGL(k_sc_svector_sum_finish_mixed, dim3(pl.n_blocks), dim3(IPAB_THREADS), 0, ctx->stream, (const u32 *)part,
                         (const u32 *)(base + pl.o_blocks), n_top, (const u32 *)d_scale, sa, sb);
  }
  HIPCHK(ctx, hipGetLastError());
  return BPMI_OK;
}

// the records assembled on the host in sorted order and uploaded, then the launches (whose wait covers this frame's buffer)
static int ipam_svector_sum(bpmi_ctx *ctx, const IpamPlan &pl, const u32 *ks, const void *d_scale, const uint8_t *xs, const uint8_t *xinvs, const uint8_t *a,
                            const uint8_t *b, const uint8_t *weights) {
  char *base = (char *)ctx->stage_in;
  const u32 P = (u32)pl.n_proofs;
  std::vector<uint8_t> recs(4 * (size_t)pl.rec_words);
  std::vector<uint64_t> first(P);                           // proof p's challenges start at pair first[p] of xs / xinvs
  uint64_t pairs = 0;
  for (u32 p = 0; p < P; p++) { first[p] = pairs; pairs += ks[p]; }
  for (u32 s = 0; s < P; s++) {
    const u32 p = pl.perm[s], k = ks[p];
    uint8_t *r = recs.data() + 4 * (size_t)pl.desc[s].rec_off;
    for (u32 j = 0; j < k; j++) { memcpy(r + 64 * j, xs + 32 * (first[p] + j), 32); memcpy(r + 64 * j + 32, xinvs + 32 * (first[p] + j), 32); }
    memcpy(r + 64 * k, a + 32 * (size_t)p, 32); memcpy(r + 64 * k + 32, b + 32 * (size_t)p, 32); memcpy(r + 64 * k + 64, weights + 32 * (size_t)p, 32);
  }
  HIPCHK(ctx, h2d(ctx, base + pl.o_rec, recs.data(), recs.size(), ctx->stream));
  const int rc = ipam_svector_launches(ctx, pl, d_scale);
  if (rc) (void)hipStreamSynchronize(ctx->stream);         // recs is owned by this frame
  return rc;
}

static bool ipam_challenges_missing(uint64_t n_proofs, const uint32_t *ks, const uint8_t *xs, const uint8_t *xinvs) {
  if (xs && xinvs) return false;
  for (uint64_t p = 0; p < n_proofs; p++) if (ks[p]) return true;
  return false;
}

int bpmi_sc_svector_sum_mixed(bpmi_ctx *ctx, uint64_t n_gens, uint64_t n_proofs, const uint32_t *ks, const uint8_t *xs, const uint8_t *xinvs, const uint8_t *a,
                              const uint8_t *b, const uint8_t *weights, const uint8_t *scale, uint8_t *sa, uint8_t *sb, uint64_t *n_top) {
  static const char *const fn = "bpmi_sc_svector_sum_mixed";
  if (!ctx || !ks || !a || !b || !weights || !sa || !sb || !n_top) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  const IpamPlan pl = ipa_mixed_plan(*ctx, n_gens, n_proofs, ks, 0, scale ? 2 : 0);
  if (pl.err) return fail(ctx, pl.err, std::string(fn) + ": " + pl.msg);
  if (ipam_challenges_missing(n_proofs, ks, xs, xinvs)) return fail(ctx, BPMI_E_ARG, "null argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = ensure_stage_in(ctx, pl.total_bytes + 512);
  if (rc) return rc;
  char *base = (char *)ctx->stage_in;
  if (scale) HIPCHK(ctx, h2d(ctx, base + pl.o_scale, scale, 32 * pl.n_top, ctx->stream));
  rc = ipam_svector_sum(ctx, pl, ks, scale ? base + pl.o_scale : nullptr, xs, xinvs, a, b, weights);
  if (rc) return rc;
  HIPCHK(ctx, hipMemcpyAsync(sa, base + pl.o_sa, 32 * pl.n_top, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(sb, base + pl.o_sb, 32 * pl.n_top, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  *n_top = pl.n_top;
  return BPMI_OK;
}

int bpmi_ipa_verify_batch_mixed_dev(bpmi_ctx *ctx, const void *d_g, const void *d_h, const void *d_hscale, uint64_t n_gens, uint64_t n_proofs, const uint32_t *ks,
                                    const uint8_t *xs, const uint8_t *xinvs, const uint8_t *a, const uint8_t *b, const uint8_t *weights, const uint8_t *extra_pts,
                                    const uint8_t *extra_scalars, uint64_t n_extra, uint8_t out[64]) {
  static const char *const fn = "bpmi_ipa_verify_batch_mixed_dev";
  if (!ctx || !d_g || !d_h || !ks || !a || !b || !weights || !out || (n_extra && (!extra_pts || !extra_scalars)))
    return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  const IpamPlan pl = ipa_mixed_plan(*ctx, n_gens, n_proofs, ks, n_extra, d_hscale ? 1 : 0);
  if (pl.err) return fail(ctx, pl.err, std::string(fn) + ": " + pl.msg);
  if (ipam_challenges_missing(n_proofs, ks, xs, xinvs)) return fail(ctx, BPMI_E_ARG, "null argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // points are checked as in bpmi_ipa_verify_batch_dev; the generators that are checked are the n_top the MSM reads
  PointCheck pc(ctx, fn, ctx->stream, ctx->opt_validate >= 1);
  const bool extra_on_host = n_extra <= VALIDATE_HOST_MAX;
  int rc;
  if (extra_on_host) { rc = pc.host(extra_pts, n_extra, "extra_pts"); if (rc) { memset(out, 0xFF, 64); return rc; } }
  rc = ensure_stage_in(ctx, pl.total_bytes + 512);
  if (rc) return rc;
  rc = ipam_svector_sum(ctx, pl, ks, d_hscale, xs, xinvs, a, b, weights);
  if (rc) return rc;
  char *base = (char *)ctx->stage_in;
  if (n_extra) {
    HIPCHK(ctx, h2d(ctx, base + pl.o_expt, extra_pts, 64 * n_extra, ctx->stream));
    HIPCHK(ctx, h2d(ctx, base + pl.o_exsc, extra_scalars, 32 * n_extra, ctx->stream));
  }
  return ipa_verify_msm(ctx, pc, d_g, d_h, pl.n_top, base + pl.o_sa, base + pl.o_sb, base + pl.o_expt, base + pl.o_exsc, n_extra, !extra_on_host, false, out);
}

}  // extern "C"
