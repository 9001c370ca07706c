// ipa_packed_mixed_dev_host.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).  HOST code.
// The batch verifier of PACKED inner-product proofs of DIFFERENT lengths (a list of classes over the prefixes of one generator list):
// bpmi_ipa_batch_prepare_mixed (the host twin, ipa_packed_host.hpp), bpmi_ipa_batch_prepare_mixed_dev and
// bpmi_ipa_verify_batch_packed_mixed_dev.  Everything the calls decide is ipa_packed_mixed_plan's (ipa_packed_mixed_plan_host.hpp); this
// file queues it: per class the uploads, per ROUND one transposition per class and ONE launch of k_ipap_roles_mixed over every class's
// row chunk, one k_ipap_finish_mixed, the status copy, the mixed s-vector launches of ipa_mixed_host.hpp from the records the kernels
// left in the workspace, and one MSM over [g[:n_top] | h[:n_top] | extra] -- no host loop over proofs.
#pragma once

// uploads, tables and preparation kernels, queued; records, extra points and extra scalars go to the given device arrays (the workspace
// regions of mp.base, or the caller's), the status bytes to the region of the plan.  `tables` must live until the stream has been waited for
static int ipapm_run(bpmi_ctx *ctx, const IpapmPlan &mp, const bpmi_ipa_packed_class *classes, const uint8_t *weights, const uint8_t *seed, u32 *d_records,
                     u32 *d_expts, u32 *d_exsc, std::vector<uint8_t> &tables) {
  char *base = (char *)ctx->stage_in;
  hipStream_t st = ctx->stream;
  std::vector<ipad::Params> par(mp.n_classes);
  for (u32 c : mp.fin_cls) {
    const IpapmClass &m = mp.cls[c];
    const uint8_t *w = weights ? weights + 32ull * ipap_weights(mp.protocol) * m.gbase : nullptr;      // the class's slice
    const int rc = ipap_stage_class(ctx, m, ipapm_class_in(classes[c], w, seed), m.k, mp.protocol, m.n_proofs, m.tr_bytes, d_records + m.rec_off,
                                    d_exsc + 8 * m.extra_off, par[c]);
    if (rc) return rc;
    par[c].gbase = m.gbase;
  }
  // the unit table (round-major), the class table of the finish and its pair offsets: one piece
  tables.assign(mp.total_bytes - mp.o_units, 0);
  auto rows_of = [&](const IpapmUnit &u, uint64_t &first, u32 &cnt) {
    const IpapmClass &m = mp.cls[u.cls];
    first = (uint64_t)u.chunk * m.rows;
    cnt = (u32)(m.n_proofs - first < m.rows ? m.n_proofs - first : m.rows);
  };
  for (size_t i = 0; i < mp.unit.size(); i++) {
    ipad::MixedUnit mu;
    memset(&mu, 0, sizeof(mu));
    mu.q = par[mp.unit[i].cls];
    uint64_t first; u32 cnt;
    rows_of(mp.unit[i], first, cnt);
    mu.q.first = first; mu.q.P_launch = cnt; mu.q.Tstride = cnt;
    mu.first_block = mp.unit[i].first_block;
    memcpy(tables.data() + (size_t)IPAPM_UNIT_STRIDE * i, &mu, sizeof(mu));
  }
  for (size_t j = 0; j < mp.fin_cls.size(); j++) {
    ipad::MixedUnit mu;
    memset(&mu, 0, sizeof(mu));
    mu.q = par[mp.fin_cls[j]];
    memcpy(tables.data() + (mp.o_fin - mp.o_units) + (size_t)IPAPM_UNIT_STRIDE * j, &mu, sizeof(mu));
  }
  memcpy(tables.data() + (mp.o_pairoff - mp.o_units), mp.pair_off.data(), mp.b_pairoff);
  HIPCHK(ctx, h2d(ctx, base + mp.o_units, tables.data(), tables.size(), st));
  {
    StageTimer t(ctx, ST_RPPREP);
    for (const IpapmRound &rd : mp.round) {
      for (u32 i = rd.first_unit; i < rd.first_unit + rd.n_units; i++) {
        const IpapmClass &m = mp.cls[mp.unit[i].cls];
        uint64_t first; u32 cnt;
        rows_of(mp.unit[i], first, cnt);
        ipap_transpose_launch(ctx, m, classes[mp.unit[i].cls].tr_off[0], first, cnt, m.W);
      }
      hipLaunchKernelGGL(ipad::k_ipap_roles_mixed, dim3(rd.blocks), dim3(64), rd.lds_bytes, st, (const uint8_t *)base + mp.o_units + (size_t)IPAPM_UNIT_STRIDE * rd.first_unit,
                         rd.n_units);
    }
    hipLaunchKernelGGL(ipad::k_ipap_finish_mixed, dim3((u32)((mp.base.n_extra + 255) / 256)), dim3(256), 0, st, (const uint8_t *)base + mp.o_fin,
                       (const u32 *)(base + mp.o_pairoff), (u32)mp.fin_cls.size(), d_expts, (uint8_t *)base + mp.o_status);
  }
  HIPCHK(ctx, hipGetLastError());
  return BPMI_OK;
}

// Protocol 1: every non-empty class's one u, on the host; the message names the class
static int ipapm_check_us(const PointCheck &pc, const IpapmPlan &mp, const bpmi_ipa_packed_class *classes) {
  if (mp.protocol != 1) return BPMI_OK;
  for (u32 c : mp.fin_cls) {
    const std::string name = "class " + std::to_string(c) + ": u";
    const int rc = pc.host(classes[c].u, 1, name.c_str());
    if (rc) return rc;
  }
  return BPMI_OK;
}
static void ipapm_rec_offsets(const IpapmPlan &mp, uint64_t *rec_byte_off) {
  for (u32 c = 0; c < mp.n_classes; c++) rec_byte_off[c] = mp.cls[c].n_proofs ? 4ull * mp.cls[c].rec_off : 0;
}

extern "C" {

int bpmi_ipa_batch_prepare_mixed(uint32_t K, int protocol, uint32_t n_classes, const bpmi_ipa_packed_class *classes, const uint8_t *weights, const uint8_t *seed,
                                 int threads, uint8_t *records, uint64_t *rec_byte_off, uint8_t *extra_pts, uint8_t *extra_scalars, uint8_t *status) {
  static const std::string fn = "bpmi_ipa_batch_prepare_mixed: ";
  const IpapmPlan mp = ipa_packed_mixed_plan(BpmiOptions(), K, protocol, n_classes, classes, weights, seed, 0, IPAP_T_BYTES_MAX);
  if (mp.err) return fail(nullptr, mp.err, fn + mp.msg);
  if (mp.empty) return BPMI_OK;
  if (!records || !rec_byte_off || !extra_pts || !extra_scalars || !status) return fail(nullptr, BPMI_E_ARG, fn + "null argument");
  if (protocol == 1)
    for (u32 c : mp.fin_cls)
      if (!ipap::point_ok(classes[c].u)) return fail(nullptr, BPMI_E_ARG, fn + "class " + std::to_string(c) + ": u[0] is not a point of the curve");
  try {
    std::vector<ipap::MixedClass> cls;
    for (u32 c : mp.fin_cls) {
      const IpapmClass &m = mp.cls[c];
      ipap::MixedClass mc;
      mc.k = m.k; mc.n_proofs = m.n_proofs; mc.gbase = m.gbase;
      mc.in = ipapm_class_in(classes[c], weights ? weights + 32ull * ipap_weights(protocol) * m.gbase : nullptr, seed);
      mc.rec = records + 4ull * m.rec_off; mc.pts = extra_pts + 64 * m.extra_off; mc.sc = extra_scalars + 32 * m.extra_off;
      cls.push_back(mc);
    }
    ipap::prepare_all_mixed(protocol, cls, threads, status);
  } catch (const std::exception &) {
    return fail(nullptr, BPMI_E_NOMEM, fn + "out of host memory");
  }
  ipapm_rec_offsets(mp, rec_byte_off);
  return BPMI_OK;
}

int bpmi_ipa_batch_prepare_mixed_dev(bpmi_ctx *ctx, uint32_t K, int protocol, uint32_t n_classes, const bpmi_ipa_packed_class *classes, const uint8_t *weights,
                                     const uint8_t *seed, void *d_records, uint64_t *rec_byte_off, void *d_extra_pts, void *d_extra_scalars, uint8_t *status) {
  static const char *const fn = "bpmi_ipa_batch_prepare_mixed_dev";
  if (!ctx) return BPMI_E_ARG;
  const IpapmPlan mp = ipa_packed_mixed_plan(*ctx, K, protocol, n_classes, classes, weights, seed, 0, ctx->ipap_t_budget ? ctx->ipap_t_budget : IPAP_T_BYTES_MAX);
  if (mp.err) return fail(ctx, mp.err, std::string(fn) + ": " + mp.msg);
  if (mp.empty) return BPMI_OK;
  if (!d_records || !rec_byte_off || !d_extra_pts || !d_extra_scalars || !status) return fail(ctx, BPMI_E_ARG, std::string(fn) + ": null argument");
  PointCheck pc(ctx, fn, ctx->stream, ctx->opt_validate >= 1);
  int rc = ipapm_check_us(pc, mp, classes);
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  rc = ensure_stage_in(ctx, mp.total_bytes + 512);
  if (rc) return rc;
  std::vector<uint8_t> tables;
  rc = ipapm_run(ctx, mp, classes, weights, seed, (u32 *)d_records, (u32 *)d_extra_pts, (u32 *)d_extra_scalars, tables);
  if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
  HIPCHK(ctx, hipMemcpyAsync(status, (char *)ctx->stage_in + mp.o_status, mp.b_status, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ipapm_rec_offsets(mp, rec_byte_off);
  return BPMI_OK;
}

int bpmi_ipa_verify_batch_packed_mixed_dev(bpmi_ctx *ctx, const void *d_g, const void *d_h, const void *d_hscale, uint64_t n_gens, int protocol, uint32_t n_classes,
                                           const bpmi_ipa_packed_class *classes, const uint8_t *weights, const uint8_t *seed, uint8_t out[64], uint8_t *status) {
  static const char *const fn = "bpmi_ipa_verify_batch_packed_mixed_dev";
  if (!ctx) return BPMI_E_ARG;
  if (!out) return fail(ctx, BPMI_E_ARG, std::string(fn) + ": null argument");
  u32 K;
  if (!log2_exact(n_gens, K) || K > IPAB_K_MAX) return fail(ctx, BPMI_E_ARG, std::string(fn) + ": n_gens must be 2^K, K <= 22");
  const IpapmPlan mp = ipa_packed_mixed_plan(*ctx, K, protocol, n_classes, classes, weights, seed, d_hscale ? 1 : 0, ctx->ipap_t_budget ? ctx->ipap_t_budget : IPAP_T_BYTES_MAX);
  if (mp.err) return fail(ctx, mp.err, std::string(fn) + ": " + mp.msg);
  if (mp.empty) { memset(out, 0, 64); return BPMI_OK; }
  if (!d_g || !d_h || !status) return fail(ctx, BPMI_E_ARG, std::string(fn) + ": null argument");
  // the proofs' points are the preparation's to check (status bit 1); the classes' u of Protocol 1 here, the first n_top generators at
  // level 2 by a kernel whose verdict is read after the MSM's own synchronisation; a refused call leaves 0xFF.. in `out`
  PointCheck pc(ctx, fn, ctx->stream, ctx->opt_validate >= 1);
  int rc = ipapm_check_us(pc, mp, classes);
  if (rc) { memset(out, 0xFF, 64); return rc; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  rc = ensure_stage_in(ctx, mp.total_bytes + 512);
  if (rc) return rc;
  char *base = (char *)ctx->stage_in;
  const IpamPlan &bp = mp.base;
  std::vector<uint8_t> tables;
  rc = ipapm_run(ctx, mp, classes, weights, seed, (u32 *)(base + bp.o_rec), (u32 *)(base + bp.o_expt), (u32 *)(base + bp.o_exsc), tables);
  if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
  HIPCHK(ctx, hipMemcpyAsync(status, base + mp.o_status, mp.b_status, hipMemcpyDeviceToHost, ctx->stream));
  rc = ipam_svector_launches(ctx, bp, d_hscale);          // (waits for the stream: `tables` and the status are done with)
  if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
  return ipa_verify_msm(ctx, pc, d_g, d_h, bp.n_top, base + bp.o_sa, base + bp.o_sb, base + bp.o_expt, base + bp.o_exsc, bp.n_extra, false, true, out);
}

// test hook: the transposition budget of the mixed packed calls of this ctx (0: the default)
int bpmi_debug_ipap_t_budget(bpmi_ctx *ctx, uint64_t bytes) {
  if (!ctx) return BPMI_E_ARG;
  ctx->ipap_t_budget = bytes;
  return BPMI_OK;
}

}  // extern "C"
