// ipa_prove_mixed_host.hpp -- part of libbpmi (included by bpmi.hip behind ipa_prove_host.hpp; one translation unit).  HOST code.
// bpmi_ipa_prove_batch_mixed and bpmi_ipa_batch_prover_commit_batch_mixed: ONE call of a batched inner-product prover over classes of
// different lengths.  The prover's tables are a capacity -- a class of n_c elements runs over g[:n_c], h[:n_c] through base lists of
// its own (ipp_class_bases) -- and every step of the protocol is the launches ipp_mixed_plan lists (ipa_prove_mixed_plan_host.hpp),
// each over all classes (ipa_prove_mixed_kernels.hpp).  The prover's buffers are used as in bpmi_ipa_prove_batch: one upload of every
// class's inputs with the call's device tables, one copy down.  Each proof is byte for byte what a prover created over the class's
// prefix writes.
#pragma once

// the lists of every class of the prover's capacity, made once per prover: *dst <- the device copy of `all`
static int ipa_mixed_lists(bpmi_ctx *ctx, const char *fn, const std::vector<unsigned short> &all, unsigned short **dst) {
  if (*dst) return BPMI_OK;
  unsigned short *dev = nullptr;
  HIPCHK(ctx, hipMalloc(&dev, 2 * all.size()));
  const hipError_t e = hipMemcpy(dev, all.data(), 2 * all.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(dev); return fail(ctx, BPMI_E_HIP, std::string(fn) + hipGetErrorString(e)); }
  *dst = dev;
  return BPMI_OK;
}

// a launch of the plan over its units: the multiplication of the classes' jobs, 2^gl lanes per job (rpp_host::launch_msm's dispatch)
static void ipa_mixed_launch_msm(hipStream_t st, const IppmLaunch &L, const rpp::MixedTab &M, const rpp::MsmJobs *jobs, const rpp::Tab &tab) {
  const dim3 grid(L.blocks), block(L.threads);
  if (L.gl == 6) hipLaunchKernelGGL(rpp::k_pv_msm_mixed<6>, grid, block, 0, st, M, jobs, tab);
  else if (L.gl == 4) hipLaunchKernelGGL(rpp::k_pv_msm_mixed<4>, grid, block, 0, st, M, jobs, tab);
  else hipLaunchKernelGGL(rpp::k_pv_msm_mixed<1>, grid, block, 0, st, M, jobs, tab);
}
#define IPM_WIDE(kern, ...)                                                                                                       \
  do {                                                                                                                            \
    if (L.threads == 256u) hipLaunchKernelGGL(ipp::kern<256>, grid, block, 0, st, __VA_ARGS__);                                   \
    else if (L.threads == 512u) hipLaunchKernelGGL(ipp::kern<512>, grid, block, 0, st, __VA_ARGS__);                              \
    else hipLaunchKernelGGL(ipp::kern<1024>, grid, block, 0, st, __VA_ARGS__);                                                    \
  } while (0)

extern "C" {

uint64_t bpmi_ipa_prove_batch_transcript_bytes_class(const bpmi_ipa_batch_prover *pv, uint32_t n, int protocol, uint64_t seed_len) {
  if (!pv || (protocol != 1 && protocol != 2) || !ipp_is_class(pv->n, n)) return 0;
  u32 k = 0;
  while ((1u << k) < n) k++;
  return ipp_transcript_bytes(k, protocol, seed_len);
}

static int ipa_prove_batch_mixed_impl(bpmi_ipa_batch_prover *pv, int protocol, uint32_t n_classes, const bpmi_ipa_prove_class *classes) {
  if (!pv) return BPMI_E_ARG;
  bpmi_ctx *ctx = pv->ctx;
  const char *fn = "bpmi_ipa_prove_batch_mixed: ";
  if (protocol != 1 && protocol != 2) return fail(ctx, BPMI_E_ARG, std::string(fn) + "protocol must be 1 or 2");
  if (n_classes == 0) return BPMI_OK;
  // ---- 1. the shapes and caps come first, from the counts alone: nothing of a call beyond them is read or allocated
  if (!classes) return fail(ctx, BPMI_E_ARG, std::string(fn) + "null argument");
  std::vector<IppmClassIn> in(n_classes <= IPPM_MAX_CLASSES ? n_classes : 0);
  for (size_t c = 0; c < in.size(); c++) { in[c].n = classes[c].n; in[c].count = classes[c].n_proofs; in[c].have_c = classes[c].c != nullptr; }
  {
    const std::string bad = ippm_args_error(pv->n, n_classes, in.data());
    if (!bad.empty()) return fail(ctx, BPMI_E_ARG, fn + bad);
  }
  auto who = [&](u32 c) { return std::string(fn) + "class " + std::to_string(c) + ": "; };
  for (u32 c = 0; c < n_classes; c++) {
    const bpmi_ipa_prove_class &k = classes[c];
    IppCall call;
    call.protocol = protocol; call.a = k.a; call.b = k.b; call.c = k.c; call.P = k.P; call.seed_off = k.seed_off; call.ab = k.ab; call.xs = k.xs; call.LR = k.LR;
    call.head = k.head; call.transcripts = k.transcripts; call.tr_off = k.tr_off;
    if (const char *bad = ipp_call_error(k.n > 1 ? 1u : 0u, call)) return fail(ctx, BPMI_E_ARG, who(c) + bad);
  }
  // ---- 2. the seeds, the plan, every class's cap
  for (u32 c = 0; c < n_classes; c++) {
    const bpmi_ipa_prove_class &k = classes[c];
    if (const char *bad = ipp_seeds_error(k.n_proofs, k.seed_off, k.seeds != nullptr, &in[c].seed_max)) return fail(ctx, BPMI_E_ARG, who(c) + bad);
  }
  const IppmPlan plan = ipp_mixed_plan(pv->n, protocol, n_classes, in.data(), ctx->opt_prover_job_lanes);
  if (plan.err) return fail(ctx, plan.err, fn + plan.msg);
  for (u32 c = 0; c < n_classes; c++)
    if (classes[c].cap < plan.cls[c].count * plan.cls[c].tr_bytes)
      return fail(ctx, BPMI_E_ARG, who(c) + "the transcript buffer is too small (n_proofs x bpmi_ipa_prove_batch_transcript_bytes_class of the longest seed)");
  // ---- 3. every scalar against q
  for (u32 c = 0; c < n_classes; c++) {
    const bpmi_ipa_prove_class &k = classes[c];
    for (int pass = 0; pass < 2; pass++)                   // a and b side by side, then c
      if (const std::string bad = pass ? rpp_host::unreduced({{"c", k.c, k.n_proofs}}) : rpp_host::unreduced({{"a", k.a, k.n_proofs * k.n}, {"b", k.b, k.n_proofs * k.n}}); !bad.empty())
        return fail(ctx, BPMI_E_ARG, who(c) + bad);
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = ipa_mixed_lists(ctx, fn, ipp_capacity_bases(pv->n), &pv->mixed_bases)) return rc;
  // ---- 4. the buffers
  const size_t in_bytes = plan.in_bytes, out_bytes = plan.need - plan.o_out;
  if (int rc = pv->mem.grow(ctx, plan.need, std::max(in_bytes, out_bytes))) return rc;
  char *d = (char *)pv->mem.buf, *hp = (char *)pv->mem.pin;
  // ---- 5. every class's staged transcript starts and inputs, the record arrays and the unit tables: one upload
  memset(hp, 0, in_bytes);
  for (u32 c = 0; c < n_classes; c++) {
    const bpmi_ipa_prove_class &k = classes[c];
    const IppmClass &q = plan.cls[c];
    const u32 P = (u32)q.count, n = q.n;
    // the transcript's start: Protocol 1 base64(seed) "&" (transcript.py:13-14), Protocol 2 "&" || prefix (inner_product_prover.py:58-63)
    for (u32 p = 0; p < P; p++) {
      uint8_t *dg = (uint8_t *)hp + q.o_dig0 + (size_t)p * q.dig0_stride;
      const uint64_t sl = k.seed_off[p + 1] - k.seed_off[p];
      size_t tl = 0;
      if (protocol == 1) { tl = rp::b64_encode(dg, sl ? k.seeds + k.seed_off[p] : (const uint8_t *)"", sl); dg[tl++] = '&'; }
      else { dg[tl++] = '&'; if (sl) memcpy(dg + tl, k.seeds + k.seed_off[p], sl); tl += sl; }
      ((u32 *)(hp + q.o_dlen))[p] = (u32)tl;
    }
    memcpy(hp + q.o_ain, k.a, 32ull * P * n);
    memcpy(hp + q.o_bin, k.b, 32ull * P * n);
    if (k.c) memcpy(hp + q.o_cin, k.c, 32ull * P);
    if (k.P) memcpy(hp + q.o_Pin, k.P, 64ull * P);
    ipp::Batch B;
    memset(&B, 0, sizeof(B));
    B.P = P; B.n = n; B.k = q.k; B.proto = (u32)protocol;
    B.dig0 = (const unsigned char *)(d + q.o_dig0); B.dig0_stride = q.dig0_stride; B.dig0_len = (const u32 *)(d + q.o_dlen);
    B.a_in = (const u32 *)(d + q.o_ain); B.b_in = (const u32 *)(d + q.o_bin);
    B.c_in = k.c ? (const u32 *)(d + q.o_cin) : nullptr; B.P_in = k.P ? (const u32 *)(d + q.o_Pin) : nullptr; B.hscale = pv->hscale;
    B.tr = (unsigned char *)(d + q.o_tr); B.tr_stride = q.tr_stride; B.tr_len = (u32 *)(d + q.o_trlen);
    B.uc = (u32 *)(d + q.o_uc); B.hsc = (u32 *)(d + q.o_hsc); B.xs = (u32 *)(d + q.o_xs); B.xr = (u32 *)(d + q.o_xr);
    B.a = (u32 *)(d + q.o_a); B.b = (u32 *)(d + q.o_b); B.cg = (u32 *)(d + q.o_cg); B.hf = (u32 *)(d + q.o_hf);
    B.jsc = (u32 *)(d + q.o_jsc); B.jout = (u32 *)(d + q.o_jout);
    B.head = (u32 *)(d + q.o_head); B.lr = (u32 *)(d + q.o_lr); B.ab = (u32 *)(d + q.o_ab);
    memcpy(hp + plan.o_batch + (size_t)IPPM_BATCH_SLOT * c, &B, sizeof(B));
    const ipp::AffineJob A = {B.jout, B.lr, 2 * P, 2u, 2 * q.k, q.k};
    memcpy(hp + plan.o_affine + (size_t)IPPM_AFFINE_SLOT * c, &A, sizeof(A));
    for (u32 s = 0; s < plan.nsteps; s++) {
      const IppmJobs &j = plan.jobs[(size_t)s * n_classes + c];
      rpp::MsmJobs J;
      memset(&J, 0, sizeof(J));
      J.njobs = j.njobs; J.ntypes = j.ntypes; J.T = j.T; J.stride = j.stride; J.out = B.jout;
      J.bases = pv->mixed_bases + q.bases_off + j.base_off;
      J.scalars = j.from_hsc ? B.hsc : B.jsc;
      memcpy(hp + plan.o_jobs + (size_t)IPPM_JOBS_SLOT * ((size_t)s * n_classes + c), &J, sizeof(J));
    }
  }
  if (!plan.units.empty()) memcpy(hp + plan.o_units, plan.units.data(), sizeof(RppmUnit) * plan.units.size());
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipMemcpyAsync(d, hp, in_bytes, hipMemcpyHostToDevice, st));
  // ---- 6. the statement points of every class in one check: their regions lie back to back, the padding between them is zero bytes
  // (the identity, a legal P)
  PointCheck pc(ctx, "bpmi_ipa_prove_batch_mixed", st, protocol == 1 && ctx->opt_validate >= 1);
  pc.queue(d + plan.o_P, (plan.o_P_end - plan.o_P) / 64, "P");
  // ---- 7. the plan's launches in order
  const rpp::Tab tab = rpp::Tab{pv->table, pv->tw, pv->wt, pv->bt};
  hipEvent_t *ev = pv->ev;
  (void)hipEventRecord(ev[0], st);
  u32 step_now = 0;
  for (const IppmLaunch &L : plan.launches) {
    if (L.step && !step_now) (void)hipEventRecord(ev[1], st);      // behind begin + first wide call (+ head): the boundary of bpmi_ipa_prove_batch
    step_now = L.step;
    const rpp::MixedTab M = {(const rpp::u8 *)(d + plan.o_batch), (const rpp::MixedUnit *)(d + plan.o_units) + L.first_unit, L.n_units};
    const dim3 grid(L.blocks), block(L.threads);
    switch (L.kind) {
      case IPPM_BEGIN: hipLaunchKernelGGL(ipp::k_ip_begin_mixed, grid, block, 0, st, M); break;
      case IPPM_ROUND_WIDE: IPM_WIDE(k_ip_round_wide_mixed, M, L.round, L.first); break;
      case IPPM_MSM: ipa_mixed_launch_msm(st, L, M, (const rpp::MsmJobs *)(d + plan.o_jobs) + (size_t)L.step * n_classes, tab); break;
      case IPPM_HEAD: hipLaunchKernelGGL(ipp::k_ip_head_mixed, grid, block, 0, st, M); break;
      case IPPM_AFFINE: hipLaunchKernelGGL(ipp::k_ip_affine_mixed, grid, block, 0, st, M, (const ipp::AffineJob *)(d + plan.o_affine), L.round); break;
      default: hipLaunchKernelGGL(ipp::k_ip_round_chal_mixed, grid, block, 0, st, M, L.round);
    }
  }
  if (!step_now) (void)hipEventRecord(ev[1], st);                  // (no class has a round)
  (void)hipEventRecord(ev[2], st);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) { int rc = pc.fetch(); if (rc) return rc; }
  // ---- 8. the proofs of every class leave through the prover's page-locked buffer, in one copy
  if (e == hipSuccess) e = hipMemcpyAsync(hp, d + plan.o_out, out_bytes, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipEventRecord(ev[3], st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(ctx, BPMI_E_HIP, std::string(fn) + hipGetErrorString(e));
  if (pc.queued && *ctx->vflag != 0xFFFFFFFFu) {                   // (no output is written) the verdict's index counts 64-byte slots from o_P
    const size_t at = plan.o_P + 64ull * (*ctx->vflag & 0x0FFFFFFFu);
    u32 c = 0;
    while (c + 1 < n_classes && plan.cls[c + 1].o_Pin <= at) c++;
    return fail(ctx, BPMI_E_ARG, who(c) + "P[" + std::to_string((at - plan.cls[c].o_Pin) / 64) + "] is not a point of the curve");
  }
  // ---- 9. the per-class copies into the caller's arrays and the transcript compaction
  const char *ho = hp - plan.o_out;                        // ho + o_x: array x in the staging buffer
  for (u32 c = 0; c < n_classes; c++) {
    const bpmi_ipa_prove_class &k = classes[c];
    const IppmClass &q = plan.cls[c];
    const u32 P = (u32)q.count;
    memcpy(k.ab, ho + q.o_ab, 64ull * P);
    if (q.k) { memcpy(k.xs, ho + q.o_xs, 32ull * P * q.k); memcpy(k.LR, ho + q.o_lr, 128ull * P * q.k); }
    if (protocol == 1) memcpy(k.head, ho + q.o_head, 128ull * P);
    uint64_t pos = 0;
    for (u32 p = 0; p < P; p++) {
      const u32 tl = ((const u32 *)(ho + q.o_trlen))[p];
      k.tr_off[p] = pos;
      memcpy(k.transcripts + pos, ho + q.o_tr + (size_t)p * q.tr_stride, tl);
      pos += tl;
    }
    k.tr_off[P] = pos;
  }
  for (int i = 0; i < 3; i++) { float ms = 0; (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]); pv->last_ms[i] = ms; }
  { float ms = 0; (void)hipEventElapsedTime(&ms, ev[0], ev[3]); pv->last_ms[3] = ms; }
  return BPMI_OK;
}
int bpmi_ipa_prove_batch_mixed(bpmi_ipa_batch_prover *pv, int protocol, uint32_t n_classes, const bpmi_ipa_prove_class *classes) {
  return rpp_host::guarded(pv ? pv->ctx : nullptr, "bpmi_ipa_prove_batch_mixed", [&] { return ipa_prove_batch_mixed_impl(pv, protocol, n_classes, classes); });
}

// The statements of the classes of a block from the prover's tables: the launches of ipp_mixed_commit_plan -- k_ip_commit_scalars_mixed per
// block size, k_pv_msm_mixed per lane width, k_ip_affine_mixed -- between one upload and one copy down of every class's points.
static int ipa_batch_prover_commit_batch_mixed_impl(bpmi_ipa_batch_prover *pv, int u_mode, uint32_t n_classes, const bpmi_ipa_commit_class *classes) {
  const char *const fn = "bpmi_ipa_batch_prover_commit_batch_mixed: ";
  if (!pv) return fail(nullptr, BPMI_E_ARG, std::string(fn) + "null argument (pv)");
  bpmi_ctx *ctx = pv->ctx;
  if (u_mode < 0 || u_mode > 2) return fail(ctx, BPMI_E_ARG, std::string(fn) + "u_mode must be 0 (no u term), 1 (t = <a, b>) or 2 (t given)");
  if (n_classes == 0) return BPMI_OK;
  if (!classes) return fail(ctx, BPMI_E_ARG, std::string(fn) + "null argument");
  std::vector<IppmClassIn> in(n_classes <= IPPM_MAX_CLASSES ? n_classes : 0);
  for (size_t c = 0; c < in.size(); c++) {
    const bpmi_ipa_commit_class &k = classes[c];
    in[c].n = k.n; in[c].count = k.count; in[c].have_a = k.a != nullptr; in[c].have_b = k.b != nullptr; in[c].have_t = k.t != nullptr;
  }
  {
    const std::string bad = ippm_args_error(pv->n, n_classes, in.data());
    if (!bad.empty()) return fail(ctx, BPMI_E_ARG, fn + bad);
  }
  auto who = [&](u32 c) { return std::string(fn) + "class " + std::to_string(c) + ": "; };
  for (u32 c = 0; c < n_classes; c++) {
    const bpmi_ipa_commit_class &k = classes[c];
    IppCommitCall call;
    call.pv = true; call.out = k.out != nullptr; call.a = k.a != nullptr; call.b = k.b != nullptr; call.t = k.t != nullptr; call.u_mode = u_mode;
    if (const char *bad = ipp_commit_error(call)) return fail(ctx, BPMI_E_ARG, who(c) + bad);
  }
  const auto wall0 = std::chrono::steady_clock::now();
  const IppmCommitPlan plan = ipp_mixed_commit_plan(pv->n, u_mode, n_classes, in.data(), ctx->opt_prover_job_lanes);
  if (plan.err) return fail(ctx, plan.err, fn + plan.msg);
  for (u32 c = 0; c < n_classes; c++) {
    const bpmi_ipa_commit_class &k = classes[c];
    for (int pass = 0; pass < 2; pass++)                   // a and b side by side, then t
      if (const std::string bad = pass ? rpp_host::unreduced({{"t", k.t, k.count}}) : rpp_host::unreduced({{"a", k.a, k.count * k.n}, {"b", k.b, k.count * k.n}}); !bad.empty())
        return fail(ctx, BPMI_E_ARG, who(c) + bad);
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = ipa_mixed_lists(ctx, fn, ipp_capacity_commit_bases(pv->n), &pv->mixed_cbases)) return rc;
  const size_t in_bytes = plan.in_bytes, out_bytes = 64 * (size_t)plan.count;
  if (int rc = pv->mem.grow(ctx, plan.need, std::max(in_bytes, out_bytes))) return rc;
  char *d = (char *)pv->mem.buf, *hp = (char *)pv->mem.pin;
  memset(hp, 0, in_bytes);
  for (u32 c = 0; c < n_classes; c++) {
    const bpmi_ipa_commit_class &k = classes[c];
    const IppmCommitClass &q = plan.cls[c];
    const u32 C = (u32)q.count, n = q.n;
    if (k.a) memcpy(hp + q.o_ain, k.a, 32ull * C * n);
    if (k.b) memcpy(hp + q.o_bin, k.b, 32ull * C * n);
    if (k.t) memcpy(hp + q.o_tin, k.t, 32ull * C);
    ipp::Commit K;
    memset(&K, 0, sizeof(K));
    K.count = C; K.n = n; K.T = q.T; K.u_mode = (u32)u_mode;
    K.a_in = k.a ? (const u32 *)(d + q.o_ain) : nullptr; K.b_in = k.b ? (const u32 *)(d + q.o_bin) : nullptr; K.t_in = k.t ? (const u32 *)(d + q.o_tin) : nullptr;
    K.hscale = pv->hscale; K.jsc = (u32 *)(d + q.o_jsc);
    memcpy(hp + plan.o_commit + (size_t)IPPM_COMMIT_SLOT * c, &K, sizeof(K));
    const ipp::AffineJob A = {(const u32 *)(d + q.o_jout), (u32 *)(d + q.o_pts), C, 1u, 1u, 0u};
    memcpy(hp + plan.o_affine + (size_t)IPPM_AFFINE_SLOT * c, &A, sizeof(A));
    rpp::MsmJobs J;
    memset(&J, 0, sizeof(J));
    J.njobs = C; J.ntypes = 1; J.T = q.T; J.stride = q.T; J.bases = pv->mixed_cbases + q.bases_off; J.scalars = K.jsc; J.out = (u32 *)(d + q.o_jout);
    memcpy(hp + plan.o_jobs + (size_t)IPPM_JOBS_SLOT * c, &J, sizeof(J));
  }
  memcpy(hp + plan.o_units, plan.units.data(), sizeof(RppmUnit) * plan.units.size());
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipMemcpyAsync(d, hp, in_bytes, hipMemcpyHostToDevice, st));
  const rpp::Tab tab = rpp::Tab{pv->table, pv->tw, pv->wt, pv->bt};
  (void)hipEventRecord(pv->ev[0], st);
  for (const IppmLaunch &L : plan.launches) {
    const rpp::MixedTab M = {(const rpp::u8 *)(d + plan.o_commit), (const rpp::MixedUnit *)(d + plan.o_units) + L.first_unit, L.n_units};
    const dim3 grid(L.blocks), block(L.threads);
    switch (L.kind) {
      case IPPM_COMMIT_SCALARS: IPM_WIDE(k_ip_commit_scalars_mixed, M); break;
      case IPPM_MSM: ipa_mixed_launch_msm(st, L, M, (const rpp::MsmJobs *)(d + plan.o_jobs), tab); break;
      default: hipLaunchKernelGGL(ipp::k_ip_affine_mixed, grid, block, 0, st, M, (const ipp::AffineJob *)(d + plan.o_affine), 0u);
    }
  }
  (void)hipEventRecord(pv->ev[1], st);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(hp, d + plan.o_out, out_bytes, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(ctx, BPMI_E_HIP, std::string(fn) + hipGetErrorString(e));
  for (u32 c = 0; c < n_classes; c++) memcpy(classes[c].out, hp + (plan.cls[c].o_pts - plan.o_out), 64 * (size_t)plan.cls[c].count);
  { float ms = 0; (void)hipEventElapsedTime(&ms, pv->ev[0], pv->ev[1]); pv->commit_ms[0] = ms; }
  pv->commit_ms[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
  return BPMI_OK;
}
int bpmi_ipa_batch_prover_commit_batch_mixed(bpmi_ipa_batch_prover *pv, int u_mode, uint32_t n_classes, const bpmi_ipa_commit_class *classes) {
  return rpp_host::guarded(pv ? pv->ctx : nullptr, "bpmi_ipa_batch_prover_commit_batch_mixed", [&] { return ipa_batch_prover_commit_batch_mixed_impl(pv, u_mode, n_classes, classes); });
}

}  // extern "C"
#undef IPM_WIDE
