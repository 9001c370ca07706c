// ipa_prove_host.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).  HOST code.
// The batched inner-product prover's object and launch sequence (kernels: ipa_prove_kernels.hpp; plan: ipa_prove_plan_host.hpp):
// bpmi_ipa_batch_prover_create builds the fixed-base tables of a generator set (u, g, h) once; bpmi_ipa_prove_batch proves any
// number of arguments over them, every protocol step as one launch over the whole batch; bpmi_ipa_batch_prover_commit_batch makes the
// statements P_p of a batch from the same tables.  ipa_prove_mixed_host.hpp (included at the end): both calls over classes of different
// lengths on one prover.
#pragma once

struct bpmi_ipa_batch_prover {
  bpmi_ctx *ctx = nullptr;
  u32 n = 0, k = 0, nbases = 0, NT = 256;
  uint64_t max_proofs = 0;
  u32 *table = nullptr;                        // [(1 + 2n)][wt][bt] affine points: base 0 u, 1 + j g_j, 1 + n + j h_j
  u32 tw = 16, wt = 16, bt = 32768;
  unsigned short *bases = nullptr;             // device: the base lists (ipp_plan)
  unsigned short *cbases = nullptr;            // device: the base lists of a statement's job (ipp_commit_bases_all)
  unsigned short *mixed_bases = nullptr;       // device: the base lists of every class n_c <= n (ipp_capacity_bases), made by the first mixed call
  unsigned short *mixed_cbases = nullptr;      // device: the statements' lists of every class (ipp_capacity_commit_bases), likewise
  u32 off_head = 0, off_round = 0;
  u32 *hscale = nullptr;                       // device: n scalars, or nullptr
  rpp_host::Buffers mem;                       // the batch's device arrays; page-locked staging of the inputs / the proofs
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};      // phase boundaries of a batch
  double last_ms[4] = {0};                     // device milliseconds of the last batch: begin + head | rounds | copy out | whole
  double commit_ms[2] = {0};                   // the last bpmi_ipa_batch_prover_commit_batch: its kernels on the device | the whole call on the host's clock
};

extern "C" {

void bpmi_ipa_batch_prover_destroy(bpmi_ipa_batch_prover *pv) {
  if (!pv) return;
  if (pv->ctx) { (void)hipSetDevice(pv->ctx->device); (void)hipStreamSynchronize(pv->ctx->stream); }
  if (pv->table) (void)hipFree(pv->table);
  if (pv->bases) (void)hipFree(pv->bases);
  if (pv->cbases) (void)hipFree(pv->cbases);
  if (pv->mixed_bases) (void)hipFree(pv->mixed_bases);
  if (pv->mixed_cbases) (void)hipFree(pv->mixed_cbases);
  if (pv->hscale) (void)hipFree(pv->hscale);
  pv->mem.release();
  for (auto e : pv->ev) if (e) (void)hipEventDestroy(e);
  delete pv;
}

static int ipa_batch_prover_create_impl(bpmi_ctx *ctx, uint32_t n, const uint8_t *g, const uint8_t *h, const uint8_t u[64], const uint8_t *h_scale,
                                        bpmi_ipa_batch_prover **out, bpmi_ipa_batch_prover *&partial) {
  if (!ctx || !g || !h || !u || !out) return ctx ? fail(ctx, BPMI_E_ARG, "null argument") : BPMI_E_ARG;
  *out = nullptr;
  const IppPlan plan = ipp_plan(n, ctx->opt_prover_tw);          // (option "prover_table_bits" is read HERE)
  if (plan.err) return fail(ctx, plan.err, plan.msg);
  if (const std::string bad = rpp_host::unreduced({{"h_scale", h_scale, n}}); !bad.empty()) return fail(ctx, BPMI_E_ARG, "bpmi_ipa_batch_prover_create: " + bad);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  {
    const PointCheck pc(ctx, "bpmi_ipa_batch_prover_create", ctx->stream, ctx->opt_validate >= 1);
    int vrc = pc.host(u, 1, "u");
    if (!vrc) vrc = pc.host(g, n, "g");
    if (!vrc) vrc = pc.host(h, n, "h");
    if (vrc) return vrc;
  }
  bpmi_ipa_batch_prover *pv = new bpmi_ipa_batch_prover();
  partial = pv;
  pv->ctx = ctx; pv->n = n; pv->k = plan.k; pv->NT = plan.NT; pv->max_proofs = plan.max_proofs; pv->nbases = plan.nbases;
  pv->tw = plan.tw; pv->wt = plan.wt; pv->bt = plan.bt;
  pv->off_head = plan.off_head; pv->off_round = plan.off_round;
  auto bail = [&](int rc) { bpmi_ipa_batch_prover_destroy(pv); partial = nullptr; return rc; };
  auto hip_fail = [&](hipError_t ee, int code) { return fail(ctx, code, std::string("bpmi_ipa_batch_prover_create: ") + hipGetErrorString(ee)); };
  for (int i = 0; i < 4; i++) { hipError_t ee = hipEventCreate(&pv->ev[i]); if (ee != hipSuccess) return bail(hip_fail(ee, BPMI_E_HIP)); }
  // the tables, with the range prover's builder
  const u32 nb = plan.nbases;
  std::vector<uint8_t> basepts(64 * (size_t)nb);
  memcpy(&basepts[0], u, 64); memcpy(&basepts[64], g, 64 * (size_t)n); memcpy(&basepts[64 + 64 * (size_t)n], h, 64 * (size_t)n);
  u32 *d_base = nullptr;
  int rc = rpp_host::build_tables(ctx, "bpmi_ipa_batch_prover_create", basepts, nb, 0, pv->tw, pv->wt, pv->bt, &d_base, &pv->table);
  hipError_t e = rc ? hipSuccess : hipStreamSynchronize(ctx->stream);
  if (d_base) (void)hipFree(d_base);
  if (rc) return bail(rc);
  if (e != hipSuccess) return bail(hip_fail(e, BPMI_E_HIP));
  const std::vector<unsigned short> &bl = plan.bases;
  e = hipMalloc(&pv->bases, 2 * bl.size());
  if (e == hipSuccess) e = hipMemcpy(pv->bases, bl.data(), 2 * bl.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    const std::vector<unsigned short> cl = ipp_commit_bases_all(n);
    e = hipMalloc(&pv->cbases, 2 * cl.size());
    if (e == hipSuccess) e = hipMemcpy(pv->cbases, cl.data(), 2 * cl.size(), hipMemcpyHostToDevice);
  }
  if (e == hipSuccess && h_scale) {
    e = hipMalloc(&pv->hscale, 32 * (size_t)n);
    if (e == hipSuccess) e = hipMemcpy(pv->hscale, h_scale, 32 * (size_t)n, hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) return bail(hip_fail(e, BPMI_E_HIP));
  *out = pv;
  partial = nullptr;
  return BPMI_OK;
}
int bpmi_ipa_batch_prover_create(bpmi_ctx *ctx, uint32_t n, const uint8_t *g, const uint8_t *h, const uint8_t u[64], const uint8_t *h_scale,
                                 bpmi_ipa_batch_prover **out) {
  bpmi_ipa_batch_prover *partial = nullptr;
  return rpp_host::guarded(ctx, "bpmi_ipa_batch_prover_create", [&] { return ipa_batch_prover_create_impl(ctx, n, g, h, u, h_scale, out, partial); },
                           [&] { if (partial) bpmi_ipa_batch_prover_destroy(partial); if (out) *out = nullptr; });
}

uint64_t bpmi_ipa_prove_batch_transcript_bytes(const bpmi_ipa_batch_prover *pv, int protocol, uint64_t seed_len) {
  if (!pv || (protocol != 1 && protocol != 2)) return 0;
  return ipp_transcript_bytes(pv->k, protocol, seed_len);
}

static int ipa_prove_batch_impl(bpmi_ipa_batch_prover *pv, int protocol, uint64_t n_proofs, const uint8_t *a, const uint8_t *b, const uint8_t *c, const uint8_t *Pst,
                                const uint8_t *seeds, const uint64_t *seed_off, uint8_t *ab, uint8_t *xs, uint8_t *LR, uint8_t *head, uint8_t *transcripts,
                                uint64_t cap, uint64_t *tr_off) {
  if (!pv) return BPMI_E_ARG;
  bpmi_ctx *ctx = pv->ctx;
  // the argument errors and the per-call caps come first: nothing of a batch beyond them is read or allocated
  IppCall call;
  call.protocol = protocol; call.a = a; call.b = b; call.c = c; call.P = Pst; call.seed_off = seed_off; call.ab = ab; call.xs = xs; call.LR = LR; call.head = head;
  call.transcripts = transcripts; call.tr_off = tr_off;
  if (n_proofs == 0) {
    if (protocol != 1 && protocol != 2) return fail(ctx, BPMI_E_ARG, "protocol must be 1 or 2");
    return BPMI_OK;
  }
  if (const char *bad = ipp_call_error(pv->k, call)) return fail(ctx, BPMI_E_ARG, std::string("bpmi_ipa_prove_batch: ") + bad);
  if (const char *over = ipp_batch_error(pv->max_proofs, n_proofs)) return fail(ctx, BPMI_E_ARG, std::string("bpmi_ipa_prove_batch: ") + over);
  uint64_t max_seed = 0;
  if (const char *bad = ipp_seeds_error(n_proofs, seed_off, seeds != nullptr, &max_seed)) return fail(ctx, BPMI_E_ARG, std::string("bpmi_ipa_prove_batch: ") + bad);
  const u32 P = (u32)n_proofs, n = pv->n, k = pv->k;
  if (const char *bad = ipp_cap_error(k, protocol, n_proofs, max_seed, cap)) return fail(ctx, BPMI_E_ARG, std::string("bpmi_ipa_prove_batch: ") + bad);
  for (int pass = 0; pass < 2; pass++)                   // a and b side by side, then c
    if (const std::string bad = pass ? rpp_host::unreduced({{"c", c, n_proofs}}) : rpp_host::unreduced({{"a", a, n_proofs * n}, {"b", b, n_proofs * n}}); !bad.empty())
      return fail(ctx, BPMI_E_ARG, "bpmi_ipa_prove_batch: " + bad);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // the transcript's start: Protocol 1 base64(seed) "&" (transcript.py:13-14), Protocol 2 "&" || prefix (inner_product_prover.py:58-63)
  const u32 dig0_stride = (u32)(((protocol == 1 ? ((max_seed + 2) / 3) * 4 + 1 : 1 + max_seed) + 15) & ~15ull);
  const u32 tr_stride = (u32)((ipp_transcript_bytes(k, protocol, max_seed) + 15) & ~15ull);
  // ---- device layout
  using rpp_host::up256;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += up256(bytes); return at; };
  const size_t o_dig0 = take((size_t)P * dig0_stride), o_dlen = take(4ull * P), o_ain = take(32ull * P * n), o_bin = take(32ull * P * n);
  const size_t o_cin = take(c ? 32ull * P : 0), o_Pin = take(Pst ? 64ull * P : 0);
  const size_t in_bytes = o;                                   // everything above is uploaded in one copy
  const size_t o_uc = take(32ull * P), o_hsc = take(64ull * P), o_xr = take(64ull * P);
  const size_t o_a = take(32ull * P * n), o_b = take(32ull * P * n), o_cg = take(32ull * P * n), o_hf = take(32ull * P * n);
  const size_t o_jsc = take(32ull * 2 * P * (n + 1)), o_jout = take(144ull * 2 * P);
  const size_t o_out = o;                                      // everything below comes back in one copy
  const size_t o_ab = take(64ull * P), o_xs = take(32ull * P * k), o_lr = take(128ull * P * k), o_head = take(128ull * P);
  const size_t o_trlen = take(4ull * P), o_tr = take((size_t)P * tr_stride);
  const size_t out_bytes = o - o_out;
  if (int rc = pv->mem.grow(ctx, o, std::max(in_bytes, out_bytes))) return rc;
  char *d = (char *)pv->mem.buf, *hp = (char *)pv->mem.pin;
  // ---- inputs into the staging buffer
  for (u32 p = 0; p < P; p++) {
    uint8_t *dg = (uint8_t *)hp + o_dig0 + (size_t)p * dig0_stride;
    const uint64_t sl = seed_off[p + 1] - seed_off[p];
    size_t tl = 0;
    if (protocol == 1) { tl = rp::b64_encode(dg, sl ? seeds + seed_off[p] : (const uint8_t *)"", sl); dg[tl++] = '&'; }
    else { dg[tl++] = '&'; if (sl) memcpy(dg + tl, seeds + seed_off[p], sl); tl += sl; }
    ((u32 *)(hp + o_dlen))[p] = (u32)tl;
  }
  memcpy(hp + o_ain, a, 32ull * P * n);
  memcpy(hp + o_bin, b, 32ull * P * n);
  if (c) memcpy(hp + o_cin, c, 32ull * P);
  if (Pst) memcpy(hp + o_Pin, Pst, 64ull * P);
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipMemcpyAsync(d, hp, in_bytes, hipMemcpyHostToDevice, st));
  PointCheck pc(ctx, "bpmi_ipa_prove_batch", st, protocol == 1 && ctx->opt_validate >= 1);
  pc.queue(d + o_Pin, P, "P");
  ipp::Batch B;
  memset(&B, 0, sizeof(B));
  B.P = P; B.n = n; B.k = k; B.proto = (u32)protocol;
  B.dig0 = (const unsigned char *)(d + o_dig0); B.dig0_stride = dig0_stride; B.dig0_len = (const u32 *)(d + o_dlen);
  B.a_in = (const u32 *)(d + o_ain); B.b_in = (const u32 *)(d + o_bin);
  B.c_in = c ? (const u32 *)(d + o_cin) : nullptr; B.P_in = Pst ? (const u32 *)(d + o_Pin) : nullptr; B.hscale = pv->hscale;
  B.tr = (unsigned char *)(d + o_tr); B.tr_stride = tr_stride; B.tr_len = (u32 *)(d + o_trlen);
  B.uc = (u32 *)(d + o_uc); B.hsc = (u32 *)(d + o_hsc); B.xs = (u32 *)(d + o_xs); B.xr = (u32 *)(d + o_xr);
  B.a = (u32 *)(d + o_a); B.b = (u32 *)(d + o_b); B.cg = (u32 *)(d + o_cg); B.hf = (u32 *)(d + o_hf);
  B.jsc = (u32 *)(d + o_jsc); B.jout = (u32 *)(d + o_jout);
  B.head = (u32 *)(d + o_head); B.lr = (u32 *)(d + o_lr); B.ab = (u32 *)(d + o_ab);
  const rpp::Tab tab = rpp::Tab{pv->table, pv->tw, pv->wt, pv->bt};
  hipEvent_t *ev = pv->ev;
  auto blocks = [](uint64_t threads, u32 per) { return dim3((u32)((threads + per - 1) / per)); };
  const u32 NT = pv->NT, per_block = NT / n;             // proofs per block of the n-lanes-per-proof kernel
  auto wide = [&](u32 round, u32 first) {
    const dim3 grid((P + per_block - 1) / per_block);
    if (NT == 256u) hipLaunchKernelGGL(ipp::k_ip_round_wide<256>, grid, dim3(256), 0, st, B, round, first);
    else if (NT == 512u) hipLaunchKernelGGL(ipp::k_ip_round_wide<512>, grid, dim3(512), 0, st, B, round, first);
    else hipLaunchKernelGGL(ipp::k_ip_round_wide<1024>, grid, dim3(1024), 0, st, B, round, first);
  };
  auto msm = [&](u32 njobs, u32 ntypes, u32 T, u32 base_off, const u32 *scalars, u32 stride, int gl) {
    rpp_host::launch_msm(st, rpp::MsmJobs{njobs, ntypes, T, pv->bases + base_off, scalars, stride, B.jout}, tab, gl);
  };
  (void)hipEventRecord(ev[0], st);
  hipLaunchKernelGGL(ipp::k_ip_begin, blocks(P, 64), dim3(64), 0, st, B);
  wide(0u, 1u);
  if (protocol == 1) {                                   // u_new = x u, P_new = P + (x c) u (inner_product_prover.py:32-33)
    msm(2 * P, 1, 1, pv->off_head, B.hsc, 1, 1);
    hipLaunchKernelGGL(ipp::k_ip_head, blocks(2ull * P, 256), dim3(256), 0, st, B);
  }
  (void)hipEventRecord(ev[1], st);
  const int job_lanes = ctx->opt_prover_job_lanes;       // 0: by the launch's job count (ipp_job_lanes_log2)
  for (u32 r = 0; r < k; r++) {                          // a round of Protocol 2 (:94-110)
    msm(2 * P, 2, n + 1, pv->off_round + r * 2 * (n + 1), B.jsc, n + 1, ipp_job_lanes_log2(n, 2 * (uint64_t)P, job_lanes));
    hipLaunchKernelGGL(rpp::k_pv_affine, blocks(2ull * P, 256), dim3(256), 0, st, (const u32 *)B.jout, 2 * P, 2u, B.lr, 2 * k, r, k);
    hipLaunchKernelGGL(ipp::k_ip_round_chal, blocks(P, 64), dim3(64), 0, st, B, r);
    wide(r, 0u);
  }
  (void)hipEventRecord(ev[2], st);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) { int rc = pc.fetch(); if (rc) return rc; }
  // the proofs leave through the prover's page-locked buffer, in one copy
  if (e == hipSuccess) e = hipMemcpyAsync(hp, d + o_out, out_bytes, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipEventRecord(ev[3], st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(ctx, BPMI_E_HIP, std::string("bpmi_ipa_prove_batch: ") + hipGetErrorString(e));
  if (int rc = pc.verdict()) return rc;                  // (no output is written)
  const char *ho = hp - o_out;                           // ho + o_x: array x in the staging buffer
  memcpy(ab, ho + o_ab, 64ull * P);
  if (k) { memcpy(xs, ho + o_xs, 32ull * P * k); memcpy(LR, ho + o_lr, 128ull * P * k); }
  if (protocol == 1) memcpy(head, ho + o_head, 128ull * P);
  uint64_t pos = 0;
  for (u32 p = 0; p < P; p++) {
    const u32 tl = ((const u32 *)(ho + o_trlen))[p];
    tr_off[p] = pos;
    memcpy(transcripts + pos, ho + o_tr + (size_t)p * tr_stride, tl);
    pos += tl;
  }
  tr_off[P] = pos;
  for (int i = 0; i < 3; i++) { float ms = 0; (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]); pv->last_ms[i] = ms; }
  { float ms = 0; (void)hipEventElapsedTime(&ms, ev[0], ev[3]); pv->last_ms[3] = ms; }
  return BPMI_OK;
}
int bpmi_ipa_prove_batch(bpmi_ipa_batch_prover *pv, int protocol, uint64_t n_proofs, const uint8_t *a, const uint8_t *b, const uint8_t *c, const uint8_t *P,
                         const uint8_t *seeds, const uint64_t *seed_off, uint8_t *ab, uint8_t *xs, uint8_t *LR, uint8_t *head, uint8_t *transcripts,
                         uint64_t cap, uint64_t *tr_off) {
  return rpp_host::guarded(pv ? pv->ctx : nullptr, "bpmi_ipa_prove_batch",
                           [&] { return ipa_prove_batch_impl(pv, protocol, n_proofs, a, b, c, P, seeds, seed_off, ab, xs, LR, head, transcripts, cap, tr_off); });
}

int bpmi_ipa_batch_prover_last_ms(const bpmi_ipa_batch_prover *pv, double ms[4]) {
  if (!pv || !ms) return BPMI_E_ARG;
  for (int i = 0; i < 4; i++) ms[i] = pv->last_ms[i];
  return BPMI_OK;
}

// The statements of a batch from the prover's tables: out[p] = sum a_p[j] g_j + sum b_p[j] (c_j h_j) + t_p u.  One upload of [a | b | t]
// through the staging buffer, k_ip_commit_scalars lays out (and under u_mode 1 sums) the rows of count jobs of one type over the base
// list of ipp_commit_bases, k_pv_msm, k_pv_affine, one copy down.  The prover's device and staging buffers are shared with proving.
static int ipa_batch_prover_commit_batch_impl(bpmi_ipa_batch_prover *pv, uint64_t count, const uint8_t *a, const uint8_t *b, int u_mode, const uint8_t *t, uint8_t *out) {
  const char *const fn = "bpmi_ipa_batch_prover_commit_batch: ";
  if (!pv) return fail(nullptr, BPMI_E_ARG, std::string(fn) + "null argument (pv)");
  bpmi_ctx *ctx = pv->ctx;
  if (count == 0) {
    if (u_mode < 0 || u_mode > 2) return fail(ctx, BPMI_E_ARG, std::string(fn) + "u_mode must be 0 (no u term), 1 (t = <a, b>) or 2 (t given)");
    return BPMI_OK;
  }
  // the argument errors and the per-call caps come first: nothing of a batch beyond them is read or allocated
  IppCommitCall call;
  call.pv = true; call.out = out != nullptr; call.a = a != nullptr; call.b = b != nullptr; call.t = t != nullptr; call.u_mode = u_mode;
  if (const char *bad = ipp_commit_error(call)) return fail(ctx, BPMI_E_ARG, std::string(fn) + bad);
  if (const char *over = ipp_batch_error(pv->max_proofs, count)) return fail(ctx, BPMI_E_ARG, std::string(fn) + over);
  const auto wall0 = std::chrono::steady_clock::now();
  const u32 C = (u32)count, n = pv->n;
  for (int pass = 0; pass < 2; pass++)                   // a and b side by side, then t
    if (const std::string bad = pass ? rpp_host::unreduced({{"t", t, count}}) : rpp_host::unreduced({{"a", a, count * n}, {"b", b, count * n}}); !bad.empty())
      return fail(ctx, BPMI_E_ARG, fn + bad);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const u32 T = (a ? n : 0u) + (b ? n : 0u) + (u_mode ? 1u : 0u);
  using rpp_host::up256;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += up256(bytes); return at; };
  const size_t o_ain = take(a ? 32ull * C * n : 0), o_bin = take(b ? 32ull * C * n : 0), o_tin = take(t ? 32ull * C : 0);
  const size_t in_bytes = o;                                   // everything above is uploaded in one copy
  const size_t o_jsc = take(32ull * C * T), o_jout = take(144ull * C), o_pts = take(64ull * C);
  if (int rc = pv->mem.grow(ctx, o, std::max(in_bytes, (size_t)(64ull * C)))) return rc;
  char *d = (char *)pv->mem.buf, *hp = (char *)pv->mem.pin;
  if (a) memcpy(hp + o_ain, a, 32ull * C * n);
  if (b) memcpy(hp + o_bin, b, 32ull * C * n);
  if (t) memcpy(hp + o_tin, t, 32ull * C);
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipMemcpyAsync(d, hp, in_bytes, hipMemcpyHostToDevice, st));
  ipp::Commit K;
  K.count = C; K.n = n; K.T = T; K.u_mode = (u32)u_mode;
  K.a_in = a ? (const u32 *)(d + o_ain) : nullptr; K.b_in = b ? (const u32 *)(d + o_bin) : nullptr; K.t_in = t ? (const u32 *)(d + o_tin) : nullptr;
  K.hscale = pv->hscale; K.jsc = (u32 *)(d + o_jsc);
  (void)hipEventRecord(pv->ev[0], st);
  const u32 NT = pv->NT;
  const dim3 grid((C + NT / n - 1) / (NT / n));
  if (NT == 256u) hipLaunchKernelGGL(ipp::k_ip_commit_scalars<256>, grid, dim3(256), 0, st, K);
  else if (NT == 512u) hipLaunchKernelGGL(ipp::k_ip_commit_scalars<512>, grid, dim3(512), 0, st, K);
  else hipLaunchKernelGGL(ipp::k_ip_commit_scalars<1024>, grid, dim3(1024), 0, st, K);
  const rpp::MsmJobs J = {C, 1, T, pv->cbases + ipp_commit_bases_offset(n, a != nullptr, b != nullptr), K.jsc, T, (u32 *)(d + o_jout)};
  rpp_host::launch_msm(st, J, rpp::Tab{pv->table, pv->tw, pv->wt, pv->bt}, ipp_job_lanes_log2(n, count, ctx->opt_prover_job_lanes));
  hipLaunchKernelGGL(rpp::k_pv_affine, dim3((C + 255u) / 256u), dim3(256), 0, st, (const u32 *)J.out, C, 1u, (u32 *)(d + o_pts), 1u, 0u, 0u);
  (void)hipEventRecord(pv->ev[1], st);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(hp, d + o_pts, 64ull * C, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(ctx, BPMI_E_HIP, std::string(fn) + hipGetErrorString(e));
  memcpy(out, hp, 64ull * C);
  { float ms = 0; (void)hipEventElapsedTime(&ms, pv->ev[0], pv->ev[1]); pv->commit_ms[0] = ms; }
  pv->commit_ms[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
  return BPMI_OK;
}
int bpmi_ipa_batch_prover_commit_batch(bpmi_ipa_batch_prover *pv, uint64_t count, const uint8_t *a, const uint8_t *b, int u_mode, const uint8_t *t, uint8_t *out) {
  return rpp_host::guarded(pv ? pv->ctx : nullptr, "bpmi_ipa_batch_prover_commit_batch", [&] { return ipa_batch_prover_commit_batch_impl(pv, count, a, b, u_mode, t, out); });
}

int bpmi_ipa_batch_prover_commit_last_ms(const bpmi_ipa_batch_prover *pv, double ms[2]) {
  if (!pv || !ms) return BPMI_E_ARG;
  ms[0] = pv->commit_ms[0]; ms[1] = pv->commit_ms[1];
  return BPMI_OK;
}

}  // extern "C"

#include "ipa_prove_mixed_host.hpp"
