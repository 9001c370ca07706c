// ipa_batch_host.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).  HOST code.
// Batch verification of inner-product proofs over shared generators: bpmi_sc_svector_sum and bpmi_ipa_verify_batch_dev.  Verifier2's
// check (/root/reference/src/innerproduct/inner_product_verifier.py:127-147) is one equation per proof; multiplied by a random weight
// each and added up, the generator terms of all proofs collapse to 2n pairs whose scalars are sums of weighted s-vectors (:91-102),
// so B proofs cost B n 2 multiplications mod q and ONE MSM of 2n + (extra pairs) instead of B MSMs of 2n.  The two equalities of
// Verifier1 (:44-58) ride along as extra pairs (innerproduct/batch.py).  Plan: ipa_batch_plan_host.hpp; kernels: scalar_kernels.hpp.
#pragma once

extern "C" {

// the half tables of every proof, from the records in the workspace.  Queued inside the CALLER's StageTimer scope: no timer of its own
static void ipab_tables_launch(bpmi_ctx *ctx, const IpabPlan &pl) {
  char *base = (char *)ctx->stage_in;
  const u32 P = (u32)pl.n_proofs, ntab = (u32)pl.tab_entries;
  const u32 gy = P < IPAB_TABLE_GRID_Y ? P : IPAB_TABLE_GRID_Y;
  hipLaunchKernelGGL(k_sc_svector_tables_batch, dim3((ntab + IPAB_THREADS - 1) / IPAB_THREADS, gy, (P + gy - 1) / gy), dim3(IPAB_THREADS), 0, ctx->stream,
                     (const u32 *)(base + pl.o_rec), pl.rec_words, pl.k, pl.kl, P, (u32 *)(base + pl.o_tab));
}

// the three launches that leave SA and SB in the workspace, from the proofs' records (k pairs (x_j, x_j^-1), then a, b, w) that are
// in the workspace already: uploaded by ipab_svector_sum, or written there by the preparation kernels (ipa_packed_dev_host.hpp)
static int ipab_svector_launches(bpmi_ctx *ctx, const IpabPlan &pl, const void *d_scale) {
  char *base = (char *)ctx->stage_in;
  u32 *sa = (u32 *)(base + pl.o_sa), *sb = (u32 *)(base + pl.o_sb), *part = (u32 *)(base + pl.o_part);
  const u32 *tabs = (const u32 *)(base + pl.o_tab);
  const u32 n = (u32)pl.n, P = (u32)pl.n_proofs, ntab = (u32)pl.tab_entries;
  {
    StageTimer t(ctx, ST_SCFOLD);
    ipab_tables_launch(ctx, pl);
    const dim3 grid((n + IPAB_THREADS - 1) / IPAB_THREADS, pl.parts);
    if (pl.direct) {
      hipLaunchKernelGGL(k_sc_svector_sum, grid, dim3(IPAB_THREADS), 0, ctx->stream, tabs, ntab, pl.kl, n, P, pl.per_part, sa, sb, (uint64_t)0);
    } else {
      hipLaunchKernelGGL(k_sc_svector_sum, grid, dim3(IPAB_THREADS), 0, ctx->stream, tabs, ntab, pl.kl, n, P, pl.per_part, part, part + 8ull * n, 16ull * n);
      hipLaunchKernelGGL(k_sc_svector_sum_finish, dim3(grid.x), dim3(IPAB_THREADS), 0, ctx->stream, (const u32 *)part, pl.parts, n, (const u32 *)d_scale, sa, sb);
    }
  }
  HIPCHK(ctx, hipGetLastError());
  return BPMI_OK;
}

// the proofs' records assembled on the host and uploaded, then the launches
static int ipab_svector_sum(bpmi_ctx *ctx, const IpabPlan &pl, const void *d_scale, const uint8_t *xs, const uint8_t *xinvs, const uint8_t *a,
                            const uint8_t *b, const uint8_t *weights) {
  char *base = (char *)ctx->stage_in;
  const u32 k = pl.k;
  const size_t rec_bytes = 4 * (size_t)pl.rec_words;
  std::vector<uint8_t> recs(rec_bytes * pl.n_proofs);
  for (uint64_t p = 0; p < pl.n_proofs; p++) {
    uint8_t *r = &recs[rec_bytes * p];
    for (u32 j = 0; j < k; j++) { memcpy(r + 64 * j, xs + 32 * (p * k + j), 32); memcpy(r + 64 * j + 32, xinvs + 32 * (p * k + j), 32); }
    memcpy(r + 64 * k, a + 32 * p, 32); memcpy(r + 64 * k + 32, b + 32 * p, 32); memcpy(r + 64 * k + 64, weights + 32 * p, 32);
  }
  HIPCHK(ctx, h2d(ctx, base + pl.o_rec, recs.data(), recs.size(), ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));          // recs is owned by this frame
  return ipab_svector_launches(ctx, pl, d_scale);
}

int bpmi_sc_svector_sum(bpmi_ctx *ctx, uint32_t k, uint64_t n_proofs, const uint8_t *xs, const uint8_t *xinvs, const uint8_t *a, const uint8_t *b,
                        const uint8_t *weights, const uint8_t *scale, uint8_t *sa, uint8_t *sb) {
  if (!ctx || !a || !b || !weights || !sa || !sb || (k && (!xs || !xinvs))) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  if (k > IPAB_K_MAX) return fail(ctx, BPMI_E_ARG, "n must be 2^k, k <= 22");
  const uint64_t n = 1ull << k;
  const IpabPlan pl = ipa_batch_plan(*ctx, n, n_proofs, 0, scale ? 2 : 0);
  if (pl.err) return fail(ctx, pl.err, std::string("bpmi_sc_svector_sum: ") + pl.msg);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = ensure_stage_in(ctx, pl.total_bytes + 512);
  if (rc) return rc;
  char *base = (char *)ctx->stage_in;
  if (scale) HIPCHK(ctx, h2d(ctx, base + pl.o_scale, scale, 32 * n, ctx->stream));
  rc = ipab_svector_sum(ctx, pl, scale ? base + pl.o_scale : nullptr, xs, xinvs, a, b, weights);
  if (rc) return rc;
  HIPCHK(ctx, hipMemcpyAsync(sa, base + pl.o_sa, 32 * n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(sb, base + pl.o_sb, 32 * n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return BPMI_OK;
}

int bpmi_ipa_verify_batch_dev(bpmi_ctx *ctx, const void *d_g, const void *d_h, const void *d_hscale, uint64_t n, uint64_t n_proofs, const uint8_t *xs,
                              const uint8_t *xinvs, uint32_t k, const uint8_t *a, const uint8_t *b, const uint8_t *weights, const uint8_t *extra_pts,
                              const uint8_t *extra_scalars, uint64_t n_extra, uint8_t out[64]) {
  static const char *const fn = "bpmi_ipa_verify_batch_dev";
  if (!ctx || !d_g || !d_h || !a || !b || !weights || !out || (k && (!xs || !xinvs)) || (n_extra && (!extra_pts || !extra_scalars)))
    return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  const IpabPlan pl = ipa_batch_plan(*ctx, n, n_proofs, n_extra, d_hscale ? 1 : 0);
  if (pl.err) return fail(ctx, pl.err, std::string(fn) + ": " + pl.msg);
  if (pl.k != k) return fail(ctx, BPMI_E_ARG, std::string(fn) + ": n must be 2^k for the k of the challenge arrays");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // points are checked as in bpmi_ipa_verify_dev: a few extra points on the host, many (and, at level 2, the generators) by a kernel
  // whose verdict is read after the MSM's own synchronisation; a refused call leaves 0xFF.. in `out`, never the identity
  PointCheck pc(ctx, fn, ctx->stream, ctx->opt_validate >= 1);
  const bool extra_on_host = n_extra <= VALIDATE_HOST_MAX;
  int rc;
  if (extra_on_host) { rc = pc.host(extra_pts, n_extra, "extra_pts"); if (rc) { memset(out, 0xFF, 64); return rc; } }
  rc = ensure_stage_in(ctx, pl.total_bytes + 512);
  if (rc) return rc;
  rc = ipab_svector_sum(ctx, pl, d_hscale, xs, xinvs, a, b, weights);
  if (rc) return rc;
  char *base = (char *)ctx->stage_in;
  if (n_extra) {
    HIPCHK(ctx, h2d(ctx, base + pl.o_expt, extra_pts, 64 * n_extra, ctx->stream));
    HIPCHK(ctx, h2d(ctx, base + pl.o_exsc, extra_scalars, 32 * n_extra, ctx->stream));
  }
  return ipa_verify_msm(ctx, pc, d_g, d_h, n, base + pl.o_sa, base + pl.o_sb, base + pl.o_expt, base + pl.o_exsc, n_extra, !extra_on_host, false, out);
}

}  // extern "C"
