// ipa_packed_dev_host.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).  HOST code.
// The batch verifier of PACKED inner-product proofs (what bpmi_ipa_prove_batch writes): bpmi_ipa_batch_prepare (the host twin,
// ipa_packed_host.hpp), bpmi_ipa_batch_prepare_dev (the kernels of ipa_packed_kernels.hpp) and bpmi_ipa_verify_batch_packed_dev:
// upload, preparation kernels, ipab_svector_launches (ipa_batch_host.hpp) from the records the kernels left in the workspace, and
// the one MSM over [g | h | extra] (ipa_verify_msm_host.hpp) -- no host loop over proofs.  Plan and argument errors:
// ipa_packed_plan_host.hpp.  The upload of a class, the description of its regions and its transposition launch stand at the top:
// the mixed and the group calls (ipa_packed_mixed_dev_host.hpp, ipa_group_dev_host.hpp) use them too, and the wire call
// (ipa_wire_dev_host.hpp) runs the kernel part, ipap_launch_kernels, over regions its expander filled.
#pragma once

// ---- what the uniform, the mixed and the group calls share: one class of proofs of one k on its way to the preparation kernels ----
// Two steps: UPLOAD the class's packed arrays into its regions, and DESCRIBE the regions to the kernels in q: everything but the rows
// of a launch (first, P_launch, Tstride) and, for a class of a mixed call, gbase.  The wire call (ipa_wire_dev_host.hpp) describes
// regions its expander filled in device memory and uploads the statements alone.  d_records / d_exsc: where the class's records and
// extra scalars go; in.weights: the class's slice of explicit weights, or NULL and in.seed.
static int ipap_upload_class(bpmi_ctx *ctx, const IpapRegions &r, const IpaPackedIn &in, uint64_t tr_bytes) {
  char *base = (char *)ctx->stage_in;
  auto up = [&](uint64_t off, const void *src, uint64_t bytes) { return bytes && src ? h2d(ctx, base + off, src, bytes, ctx->stream) : hipSuccess; };
  HIPCHK(ctx, up(r.o_ab, in.ab, r.b_ab));
  HIPCHK(ctx, up(r.o_xs, in.xs, r.b_xs));
  HIPCHK(ctx, up(r.o_lr, in.LR, r.b_lr));
  HIPCHK(ctx, up(r.o_tr, in.transcripts ? in.transcripts + in.tr_off[0] : nullptr, tr_bytes));
  HIPCHK(ctx, up(r.o_troff, in.tr_off, r.b_troff));
  HIPCHK(ctx, up(r.o_start, in.start, r.b_start));
  HIPCHK(ctx, up(r.o_u, in.u, r.b_u));
  HIPCHK(ctx, up(r.o_P, in.P, r.b_P));
  HIPCHK(ctx, up(r.o_c, in.c, r.b_c));
  HIPCHK(ctx, up(r.o_head, in.head, r.b_head));
  HIPCHK(ctx, up(r.o_w, in.weights, r.b_w));
  return BPMI_OK;
}
// has_start: the start region holds one word per proof (else 1 / 3 for every proof); weights / seed: the class's explicit weights were
// uploaded into their region, or NULL and the 32 seed bytes
static void ipap_describe_class(bpmi_ctx *ctx, const IpapRegions &r, bool has_start, const uint8_t *weights, const uint8_t *seed, u32 k, int protocol,
                                uint64_t n_proofs, u32 *d_records, u32 *d_exsc, ipad::Params &q) {
  char *base = (char *)ctx->stage_in;
  memset(&q, 0, sizeof(q));
  q.tr_off = (const u64 *)(base + r.o_troff);
  q.start = has_start ? (const u32 *)(base + r.o_start) : nullptr;
  q.ab = (const uint8_t *)base + r.o_ab; q.xs = (const uint8_t *)base + r.o_xs; q.LR = (const uint8_t *)base + r.o_lr;
  q.u = (const uint8_t *)base + r.o_u; q.P = (const uint8_t *)base + r.o_P; q.c = (const uint8_t *)base + r.o_c; q.head = (const uint8_t *)base + r.o_head;
  q.weights = weights ? (const uint8_t *)base + r.o_w : nullptr;
  if (!weights)
    for (int i = 0; i < 8; i++) q.seed[i] = ((u32)seed[4 * i] << 24) | ((u32)seed[4 * i + 1] << 16) | ((u32)seed[4 * i + 2] << 8) | seed[4 * i + 3];
  q.k = k; q.protocol = (u32)protocol; q.Pall = (u32)n_proofs; q.validate = ctx->opt_validate >= 1 ? 1u : 0u;
  q.records = d_records; q.extra_sc = d_exsc; q.roles = (uint8_t *)base + r.o_roles;
  q.T = (const u64 *)(base + r.o_T);
}
static int ipap_stage_class(bpmi_ctx *ctx, const IpapRegions &r, const IpaPackedIn &in, u32 k, int protocol, uint64_t n_proofs, uint64_t tr_bytes,
                            u32 *d_records, u32 *d_exsc, ipad::Params &q) {
  const int rc = ipap_upload_class(ctx, r, in, tr_bytes);
  if (rc) return rc;
  ipap_describe_class(ctx, r, in.start != nullptr, in.weights, in.seed, k, protocol, n_proofs, d_records, d_exsc, q);
  return BPMI_OK;
}
// the class's transcripts of proofs [first, first + cnt) into its T region; tr_off0: the host's tr_off[0], where the upload began
static void ipap_transpose_launch(bpmi_ctx *ctx, const IpapRegions &r, uint64_t tr_off0, uint64_t first, u32 cnt, u32 W) {
  char *base = (char *)ctx->stage_in;
  hipLaunchKernelGGL(ipad::k_ipap_transpose, dim3((cnt + 63) / 64, (W + 63) / 64), dim3(256), 0, ctx->stream, (const uint8_t *)base + r.o_tr,
                     (const u64 *)(base + r.o_troff) + first, tr_off0, cnt, W, (u32)IPAP_MAX_TRANSCRIPT, (u64 *)(base + r.o_T));
}

// The kernel part of one uniform class whose regions q describes: per launch of at most `rows` proofs fill(first, cnt) leaves the
// launch's transcripts in T (the transposition of the uploaded bytes, or the wire expander), k_ipap_roles runs, after_roles(first, cnt)
// may add verdicts of its own to the role bytes; then k_ipap_finish over every pair.  The status bytes go to d_status.
template <class Fill, class AfterRoles>
static int ipap_launch_kernels(bpmi_ctx *ctx, ipad::Params &q, u32 rows, u32 pairs, u32 *d_expts, uint8_t *d_status, Fill fill, AfterRoles after_roles) {
  hipStream_t st = ctx->stream;
  const uint64_t P = q.Pall;
  {
    StageTimer t(ctx, ST_RPPREP);
    for (uint64_t first = 0; first < P; first += rows) {
      const u32 cnt = (u32)(P - first < rows ? P - first : rows);
      q.first = first; q.P_launch = cnt; q.Tstride = cnt;
      fill(first, cnt);
      hipLaunchKernelGGL(ipad::k_ipap_roles, dim3(IPAP_ROLES * ((cnt + 63) / 64)), dim3(64), (size_t)q.k * 9 * 64 * 4, st, q);
      after_roles(first, cnt);
    }
    const uint64_t pairs_all = P * pairs;
    hipLaunchKernelGGL(ipad::k_ipap_finish, dim3((u32)((pairs_all + 255) / 256)), dim3(256), 0, st, q, pairs, d_expts, d_status);
  }
  HIPCHK(ctx, hipGetLastError());
  return BPMI_OK;
}
// upload the packed arrays into their regions and run the preparation kernels; records, extra points and extra scalars go to the
// given device arrays (the workspace regions of pl.base, or the caller's), the status bytes to the region of the plan
static int ipap_run(bpmi_ctx *ctx, const IpapPlan &pl, const IpaPackedIn &in, u32 *d_records, u32 *d_expts, u32 *d_exsc) {
  char *base = (char *)ctx->stage_in;
  ipad::Params q;
  const int rc = ipap_stage_class(ctx, pl, in, pl.base.k, pl.protocol, pl.base.n_proofs, pl.tr_bytes, d_records, d_exsc, q);
  if (rc) return rc;
  return ipap_launch_kernels(ctx, q, pl.rows, pl.pairs, d_expts, (uint8_t *)base + pl.o_status,
                             [&](uint64_t first, u32 cnt) { ipap_transpose_launch(ctx, pl, in.tr_off[0], first, cnt, pl.W); }, [](uint64_t, u32) {});
}

extern "C" {

int bpmi_ipa_batch_prepare(uint32_t k, int protocol, uint64_t n_proofs, const uint8_t *ab, const uint8_t *xs, const uint8_t *LR, const uint8_t *transcripts,
                           const uint64_t *tr_off, const uint32_t *start, const uint8_t *u, const uint8_t *P, const uint8_t *c, const uint8_t *head,
                           const uint8_t *weights, const uint8_t *seed, int threads, uint8_t *records, uint8_t *extra_pts, uint8_t *extra_scalars,
                           uint8_t *status) {
  static const std::string fn = "bpmi_ipa_batch_prepare: ";
  if (n_proofs == 0) return BPMI_OK;
  if (!records || !extra_pts || !extra_scalars || !status) return fail(nullptr, BPMI_E_ARG, fn + "null argument");
  const IpaPackedIn in = ipap_in(ab, xs, LR, transcripts, tr_off, start, u, P, c, head, weights, seed);
  const IpapPlan pl = ipa_packed_plan(BpmiOptions(), k, protocol, n_proofs, in, 0);
  if (pl.err) return fail(nullptr, pl.err, fn + pl.msg);
  if (protocol == 1 && !ipap::point_ok(u)) return fail(nullptr, BPMI_E_ARG, fn + "u[0] is not a point of the curve");
  try {
    ipap::prepare_all(k, protocol, n_proofs, in, threads, records, extra_pts, extra_scalars, status);
  } catch (const std::exception &) {
    return fail(nullptr, BPMI_E_NOMEM, fn + "out of host memory");
  }
  return BPMI_OK;
}

int bpmi_ipa_batch_prepare_dev(bpmi_ctx *ctx, uint32_t k, int protocol, uint64_t n_proofs, const uint8_t *ab, const uint8_t *xs, const uint8_t *LR,
                               const uint8_t *transcripts, const uint64_t *tr_off, const uint32_t *start, const uint8_t *u, const uint8_t *P, const uint8_t *c,
                               const uint8_t *head, const uint8_t *weights, const uint8_t *seed, void *d_records, void *d_extra_pts, void *d_extra_scalars,
                               uint8_t *status) {
  static const char *const fn = "bpmi_ipa_batch_prepare_dev";
  if (!ctx) return BPMI_E_ARG;
  if (n_proofs == 0) return BPMI_OK;
  if (!d_records || !d_extra_pts || !d_extra_scalars || !status) return fail(ctx, BPMI_E_ARG, std::string(fn) + ": null argument");
  const IpaPackedIn in = ipap_in(ab, xs, LR, transcripts, tr_off, start, u, P, c, head, weights, seed);
  const IpapPlan pl = ipa_packed_plan(*ctx, k, protocol, n_proofs, in, 0);
  if (pl.err) return fail(ctx, pl.err, std::string(fn) + ": " + pl.msg);
  PointCheck pc(ctx, fn, ctx->stream, ctx->opt_validate >= 1);
  int rc = protocol == 1 ? pc.host(u, 1, "u") : BPMI_OK;
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  rc = ensure_stage_in(ctx, pl.total_bytes + 512);
  if (rc) return rc;
  rc = ipap_run(ctx, pl, in, (u32 *)d_records, (u32 *)d_extra_pts, (u32 *)d_extra_scalars);
  if (rc) return rc;
  HIPCHK(ctx, hipMemcpyAsync(status, (char *)ctx->stage_in + pl.o_status, n_proofs, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return BPMI_OK;
}

int bpmi_ipa_verify_batch_packed_dev(bpmi_ctx *ctx, const void *d_g, const void *d_h, const void *d_hscale, uint64_t n, int protocol, uint64_t n_proofs,
                                     const uint8_t *ab, const uint8_t *xs, const uint8_t *LR, const uint8_t *transcripts, const uint64_t *tr_off,
                                     const uint32_t *start, const uint8_t *u, const uint8_t *P, const uint8_t *c, const uint8_t *head, const uint8_t *weights,
                                     const uint8_t *seed, uint8_t out[64], uint8_t *status) {
  static const char *const fn = "bpmi_ipa_verify_batch_packed_dev";
  if (!ctx) return BPMI_E_ARG;
  if (!out) return fail(ctx, BPMI_E_ARG, std::string(fn) + ": null argument");
  if (n_proofs == 0) { memset(out, 0, 64); return BPMI_OK; }
  if (!d_g || !d_h || !status) return fail(ctx, BPMI_E_ARG, std::string(fn) + ": null argument");
  u32 k;
  if (!log2_exact(n, k) || k > IPAB_K_MAX) return fail(ctx, BPMI_E_ARG, std::string(fn) + ": n must be 2^k, k <= 22");
  const IpaPackedIn in = ipap_in(ab, xs, LR, transcripts, tr_off, start, u, P, c, head, weights, seed);
  const IpapPlan pl = ipa_packed_plan(*ctx, k, protocol, n_proofs, in, d_hscale ? 1 : 0);
  if (pl.err) return fail(ctx, pl.err, std::string(fn) + ": " + pl.msg);
  // the proofs' points are the preparation's to check (status bit 1); the shared u of Protocol 1 here, the generators at level 2
  // by a kernel whose verdict is read after the MSM's own synchronisation; a refused call leaves 0xFF.. in `out`
  PointCheck pc(ctx, fn, ctx->stream, ctx->opt_validate >= 1);
  int rc = protocol == 1 ? pc.host(u, 1, "u") : BPMI_OK;
  if (rc) { memset(out, 0xFF, 64); return rc; }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  rc = ensure_stage_in(ctx, pl.total_bytes + 512);
  if (rc) return rc;
  char *base = (char *)ctx->stage_in;
  const IpabPlan &bp = pl.base;
  rc = ipap_run(ctx, pl, in, (u32 *)(base + bp.o_rec), (u32 *)(base + bp.o_expt), (u32 *)(base + bp.o_exsc));
  if (rc) return rc;
  HIPCHK(ctx, hipMemcpyAsync(status, base + pl.o_status, n_proofs, hipMemcpyDeviceToHost, ctx->stream));
  rc = ipab_svector_launches(ctx, bp, d_hscale);
  if (rc) return rc;
  return ipa_verify_msm(ctx, pc, d_g, d_h, n, base + bp.o_sa, base + bp.o_sb, base + bp.o_expt, base + bp.o_exsc, bp.n_extra, false, true, out);
}

}  // extern "C"
