// rp_prove_mixed_host.hpp -- part of libbpmi (included by bpmi.hip behind rp_prove_host.hpp; one translation unit).  HOST code.
// bpmi_rp_prove_batch_mixed: ONE call of a prover over classes of different sizes.  The prover's tables are a capacity -- a class of m_c
// values per proof runs over the first nbits m_c of gs and of hs through base lists of its own (rpp_class_bases) -- and every step of
// the protocol is the launches rpp_mixed_plan lists (rp_prove_mixed_plan_host.hpp), each over all classes (rp_prove_mixed_kernels.hpp).
// The prover's buffers are used as in bpmi_rp_prove_batch: one upload of every class's inputs with the call's device tables, one copy
// down, straight into a page-locked `out`.  Each proof is byte for byte what a prover created over the class's prefix writes.
#pragma once

extern "C" {

uint64_t bpmi_rp_prove_batch_proof_bytes_class(const bpmi_rp_prover *pv, uint32_t m, uint64_t seed_len) {
  if (!pv || m < 1 || (m & (m - 1)) || m > pv->m || (uint64_t)pv->nb * m < 2) return 0;
  return rpp_fixed_bytes(rpp_geom(pv->nb, m).k, pv->ctx->opt_prover_wire) + seed_len;
}

static int rp_prove_batch_mixed_impl(bpmi_rp_prover *pv, uint32_t n_classes, const bpmi_rp_prove_class *classes, uint8_t *out, uint64_t cap, uint64_t *out_off) {
  if (!pv) return BPMI_E_ARG;
  bpmi_ctx *ctx = pv->ctx;
  const char *fn = "bpmi_rp_prove_batch_mixed: ";
  if (!out || !out_off || (n_classes && !classes)) return fail(ctx, BPMI_E_ARG, std::string(fn) + "null argument");
  if (n_classes == 0) { out_off[0] = 0; return BPMI_OK; }
  // the caps and shapes come first, from the counts alone: nothing of a call beyond them is read or allocated
  std::vector<RppmClassIn> in(n_classes <= RPPM_MAX_CLASSES ? n_classes : 0);
  for (size_t c = 0; c < in.size(); c++) { in[c].m = classes[c].m; in[c].count = classes[c].n_proofs; }
  {
    const std::string bad = rppm_args_error(pv->nb, pv->m, n_classes, in.data());
    if (!bad.empty()) return fail(ctx, BPMI_E_ARG, fn + bad);
  }
  for (u32 c = 0; c < n_classes; c++) {
    const bpmi_rp_prove_class &k = classes[c];
    const std::string who = std::string(fn) + "class " + std::to_string(c) + ": ";
    if (!k.values || !k.gammas || !k.seed_off) return fail(ctx, BPMI_E_ARG, who + "null argument");
    for (uint64_t p = 0; p < k.n_proofs; p++) {
      if (k.seed_off[p + 1] < k.seed_off[p]) return fail(ctx, BPMI_E_ARG, who + "seed offsets must not decrease");
      const uint64_t sl = k.seed_off[p + 1] - k.seed_off[p];
      if (sl > 0xFFFF) return fail(ctx, BPMI_E_ARG, who + "a seed is longer than 65535 bytes");
      in[c].seed_max = std::max(in[c].seed_max, sl);
    }
    in[c].seed_total = k.seed_off[k.n_proofs] - k.seed_off[0];
    if (!k.seeds && in[c].seed_total) return fail(ctx, BPMI_E_ARG, who + "null argument");
  }
  const int wire_fmt = ctx->opt_prover_wire;
  const RppmPlan plan = rpp_mixed_plan(pv->nb, pv->m, pv->tw, n_classes, in.data(), wire_fmt, ctx->opt_prover_job_lanes, pv->ip_prefix.size());
  if (plan.err) return fail(ctx, plan.err, fn + plan.msg);
  if (plan.total_out > cap) return fail(ctx, BPMI_E_ARG, std::string(fn) + "the output buffer is too small (bpmi_rp_prove_batch_proof_bytes_class per proof)");
  for (u32 c = 0; c < n_classes; c++) {
    const bpmi_rp_prove_class &k = classes[c];
    if (const std::string bad = rpp_host::unreduced({{"values", k.values, k.n_proofs * k.m}, {"gammas", k.gammas, k.n_proofs * k.m}}); !bad.empty())
      return fail(ctx, BPMI_E_ARG, std::string(fn) + "class " + std::to_string(c) + ": " + bad);
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // the base lists of every class of this capacity, once per prover
  if (!pv->mixed_bases) {
    std::vector<unsigned short> all;
    for (u32 m = 1; m <= pv->m; m <<= 1) {
      if (pv->nb * m < 2) continue;
      const std::vector<unsigned short> bl = rpp_class_bases(pv->nb * m, pv->n);
      all.insert(all.end(), bl.begin(), bl.end());
    }
    unsigned short *dev = nullptr;
    HIPCHK(ctx, hipMalloc(&dev, 2 * all.size()));
    const hipError_t e = hipMemcpy(dev, all.data(), 2 * all.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(dev); return fail(ctx, BPMI_E_HIP, std::string(fn) + hipGetErrorString(e)); }
    pv->mixed_bases = dev;
  }
  const size_t total_out = (size_t)plan.total_out, in_bytes = plan.in_bytes;
  if (int rc = pv->mem.grow(ctx, plan.need, std::max(in_bytes, total_out))) return rc;        // (the output half is only used when `out` is pageable)
  char *d = (char *)pv->mem.buf, *hp = (char *)pv->mem.pin;
  // ---- every class's inputs and the call's device tables into the staging buffer
  memset(hp, 0, in_bytes);
  uint64_t *soff = (uint64_t *)(hp + plan.o_soff), *ooff = (uint64_t *)(hp + plan.o_ooff);
  const rpp::Tab tab = rpp::Tab{pv->table, pv->tw, pv->wt, pv->bt};
  for (u32 c = 0; c < n_classes; c++) {
    const bpmi_rp_prove_class &k = classes[c];
    const RppmClass &q = plan.cls[c];
    rpp_host::stage_inputs(hp, q, q, q.m, (u32)q.count, k.values, k.gammas, k.seeds, k.seed_off, hp + plan.o_seeds + q.seed_at, soff + q.first, ooff + q.first, q.seed_at,
                           q.out_at, q.fixed_bytes);
    const rpp::Batch B = rpp_host::make_batch(pv, d, q, q, (u32)q.count, q, 3 + pv->n, (u32)q.first);
    memcpy(hp + plan.o_batch + (size_t)RPPM_BATCH_SLOT * c, &B, sizeof(B));
    for (u32 s = 0; s + 1 < plan.nsteps; s++) {
      const RppmJobs &j = plan.jobs[(size_t)s * n_classes + c];
      rpp::MsmJobs J;
      memset(&J, 0, sizeof(J));
      J.njobs = j.njobs; J.ntypes = j.ntypes; J.T = j.T; J.stride = j.stride; J.out = B.jout;
      J.bases = pv->mixed_bases + q.bases_off + j.base_off;
      J.scalars = j.from_slr ? B.slr : j.from_tsc ? B.tsc : B.jsc;
      memcpy(hp + plan.o_jobs + (size_t)RPPM_JOBS_SLOT * ((size_t)s * n_classes + c), &J, sizeof(J));
    }
  }
  if (!plan.units.empty()) memcpy(hp + plan.o_units, plan.units.data(), sizeof(RppmUnit) * plan.units.size());
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipMemcpyAsync(d, hp, in_bytes, hipMemcpyHostToDevice, st));
  // ---- the steps: the plan's launches in order
  hipEvent_t *ev = pv->ev;
  (void)hipEventRecord(ev[0], st);
  u32 step_now = 0;
  for (const RppmLaunch &L : plan.launches) {
    // the phase boundaries of bpmi_rp_prover_last_ms: behind step 0, behind step 1, behind P_new's points, before the wire bytes
    for (; step_now < L.step; step_now++) if (step_now < 2) (void)hipEventRecord(ev[step_now + 1], st);
    if (L.kind == RPPM_EMIT) (void)hipEventRecord(ev[4], st);
    const rpp::MixedTab M = {(const rpp::u8 *)(d + plan.o_batch), (const rpp::MixedUnit *)(d + plan.o_units) + L.first_unit, L.n_units};
    const dim3 grid(L.blocks), block(L.threads);
#define PVM_WIDE(kern, ...)                                                                                                       \
  do {                                                                                                                            \
    if (L.threads == 256u) hipLaunchKernelGGL(rpp::kern<256>, grid, block, 0, st, __VA_ARGS__);                                   \
    else if (L.threads == 512u) hipLaunchKernelGGL(rpp::kern<512>, grid, block, 0, st, __VA_ARGS__);                              \
    else hipLaunchKernelGGL(rpp::kern<1024>, grid, block, 0, st, __VA_ARGS__);                                                    \
  } while (0)
    switch (L.kind) {
      case RPPM_BLIND: hipLaunchKernelGGL(rpp::k_pv_blind_mixed, grid, block, 0, st, M); break;
      case RPPM_COMMIT_A: hipLaunchKernelGGL(rpp::k_pv_commit_A_mixed, grid, block, 0, st, M); break;
      case RPPM_AFFINE:
        hipLaunchKernelGGL(rpp::k_pv_affine_mixed, grid, block, 0, st, M, L.per, L.slot0, L.slot_step, L.step_k);
        if (L.step == 2) (void)hipEventRecord(ev[3], st);
        break;
      case RPPM_MSM: {
        const rpp::MsmJobs *jobs = (const rpp::MsmJobs *)(d + plan.o_jobs) + (size_t)L.step * n_classes;
        if (L.gl == 6) hipLaunchKernelGGL(rpp::k_pv_msm_mixed<6>, grid, block, 0, st, M, jobs, tab);
        else if (L.gl == 4) hipLaunchKernelGGL(rpp::k_pv_msm_mixed<4>, grid, block, 0, st, M, jobs, tab);
        else hipLaunchKernelGGL(rpp::k_pv_msm_mixed<1>, grid, block, 0, st, M, jobs, tab);
        break;
      }
      case RPPM_CHAL_YZ: hipLaunchKernelGGL(rpp::k_pv_chal_yz_mixed, grid, block, 0, st, M); break;
      case RPPM_POLY: PVM_WIDE(k_pv_poly_mixed, M); break;
      case RPPM_FINAL_CHAL: hipLaunchKernelGGL(rpp::k_pv_final_chal_mixed, grid, block, 0, st, M); break;
      case RPPM_FINAL_WIDE: PVM_WIDE(k_pv_final_wide_mixed, M); break;
      case RPPM_ROUND_WIDE: PVM_WIDE(k_pv_round_wide_mixed, M, L.round, L.first); break;
      case RPPM_ROUND_CHAL: hipLaunchKernelGGL(rpp::k_pv_round_chal_mixed, grid, block, 0, st, M, L.round); break;
      default:
        hipLaunchKernelGGL(rpp::k_pv_emit_mixed, grid, block, 0, st, M, (const unsigned char *)(d + plan.o_seeds), (const uint64_t *)(d + plan.o_soff),
                           (unsigned char *)(d + plan.o_out), (const uint64_t *)(d + plan.o_ooff), (u32)wire_fmt);
    }
#undef PVM_WIDE
  }
  // the output offsets leave the staging buffer before the proofs may land in it
  const std::vector<uint64_t> offs(ooff, ooff + plan.n_proofs + 1);
  if (int rc = rpp_host::finish_call(pv, fn, d + plan.o_out, total_out, out)) return rc;
  memcpy(out_off, offs.data(), 8 * offs.size());
  return BPMI_OK;
}

int bpmi_rp_prove_batch_mixed(bpmi_rp_prover *pv, uint32_t n_classes, const bpmi_rp_prove_class *classes, uint8_t *out, uint64_t cap, uint64_t *out_off) {
  return rpp_host::guarded(pv ? pv->ctx : nullptr, "bpmi_rp_prove_batch_mixed", [&] { return rp_prove_batch_mixed_impl(pv, n_classes, classes, out, cap, out_off); });
}

}  // extern "C"
