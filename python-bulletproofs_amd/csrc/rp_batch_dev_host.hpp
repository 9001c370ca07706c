// rp_batch_dev_host.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).  HOST code.
// The batch verifier of range proofs: the host-side preparation (bpmi_rp_batch_prepare, whose algorithm is rp_batch_host.hpp's) and
// the device path -- bpmi_rp_batch_prepare_dev, bpmi_rp_batch_verify_dev, bpmi_rp_batch_group_values_dev.  Everything the device
// path DECIDES (argument errors, buffer layouts, rows, slices, launch shapes) is rp_prepare_plan's, rp_batch_plan_host.hpp;
// rp_prepare_enqueue is a driver that queues the plan's stages on the ctx's two lanes.  Kernels: rp_batch_kernels.hpp,
// point_kernels.hpp (the point decoding), msm_kernels.hpp (the groups' MSMs).
#pragma once

extern "C" {

// ---- batch verification of range proofs: host-side preparation ---------------------------------------
int bpmi_rp_batch_prepare(uint32_t n_gens, uint32_t values_per_proof, uint64_t n_proofs, const uint8_t *blobs, uint64_t blobs_len, const uint64_t *blob_off,
                          const uint8_t *weights, const uint8_t *seed, int threads, uint8_t *v_scalars, uint8_t *pt_scalars, uint8_t *shared, uint8_t *comp_out,
                          int64_t *first_bad) {
  if (!blobs || !blob_off || (!weights && !seed) || !v_scalars || !pt_scalars || !shared || !first_bad) return BPMI_E_ARG;
  if (n_gens < 2 || (n_gens & (n_gens - 1)) || n_gens > 65536) return BPMI_E_ARG;
  const uint32_t m = values_per_proof;
  if (m < 1 || n_gens % m) return BPMI_E_ARG;
  uint32_t k = 0;
  while ((1u << k) < n_gens) k++;
  *first_bad = -1;
  // the offset table comes from the caller, the proofs from the network: never read outside blobs[0, blobs_len)
  if (blob_off[0] > blobs_len) return BPMI_E_ARG;
  for (uint64_t g = 0; g < n_proofs; g++) if (blob_off[g] > blob_off[g + 1] || blob_off[g + 1] > blobs_len) return BPMI_E_ARG;
  // wire formats 2 and 3 (rp_wire_v2_host.hpp): expanded to format 1 here (format 3's y coordinates checked), then everything below
  // runs as before
  std::vector<uint8_t> expanded;
  std::vector<uint64_t> expanded_off;
  bool any_v2 = false;
  for (uint64_t g = 0; g < n_proofs && !any_v2; g++)
    any_v2 = blob_off[g + 1] >= blob_off[g] + 5 && (blobs[blob_off[g] + 4] == '2' || blobs[blob_off[g] + 4] == '3');
  if (any_v2) {
    expanded_off.assign(n_proofs + 1, 0);
    std::vector<uint8_t> one;
    for (uint64_t g = 0; g < n_proofs; g++) {
      const uint8_t *b = blobs + blob_off[g];
      const size_t len = (size_t)(blob_off[g + 1] - blob_off[g]);
      // a format-1 proof among format-2 ones is taken as it is; so is a blob that claims format 2 and does not expand -- it is not a
      // format-1 proof either, so the checks below reject it AT ITS INDEX, behind any earlier bad proof (returning here at once made
      // the host name a later proof than the device: tools/fuzz_batch_prepare.py, round 5)
      if (len >= 5 && (b[4] == '2' || b[4] == '3') && rpw::expand_v2(b, len, one)) expanded.insert(expanded.end(), one.begin(), one.end());
      else expanded.insert(expanded.end(), b, b + len);
      expanded_off[g + 1] = expanded.size();
    }
    blobs = expanded.data(); blobs_len = expanded.size(); blob_off = expanded_off.data();
  }
  const size_t nacc = 5 + 2 * (size_t)n_gens;
  if (threads < 1) threads = 1;
  if ((uint64_t)threads > n_proofs) threads = n_proofs ? (int)n_proofs : 1;
  std::vector<uint64_t> pt_off(n_proofs + 1);
  for (uint64_t g = 0; g <= n_proofs; g++) pt_off[g] = g * (6 + 2 * (uint64_t)k);
  std::vector<std::vector<rp::Sq>> acc(threads, std::vector<rp::Sq>(nacc, rp::q_small(0)));
  std::vector<uint64_t> bad(threads, UINT64_MAX);
  auto work = [&](int t) {
    const uint64_t lo = n_proofs * t / threads, hi = n_proofs * (t + 1) / threads;
    // sub-chunks bound the scratch memory and keep one modular inversion per ~512 proofs
    for (uint64_t a = lo; a < hi; a += 512) {
      const uint64_t b = a + 512 < hi ? a + 512 : hi;
      uint64_t bd = UINT64_MAX;
      if (!rp::run_chunk(n_gens, k, m, blobs, blob_off, weights, a, b, pt_off.data(), v_scalars, pt_scalars, comp_out, acc[t].data(), &bd, seed)) { bad[t] = bd; return; }
    }
  };
  if (threads == 1) work(0);
  else {
    std::vector<std::thread> th;
    for (int t = 0; t < threads; t++) th.emplace_back(work, t);
    for (auto &x : th) x.join();
  }
  for (int t = 0; t < threads; t++) if (bad[t] != UINT64_MAX && (*first_bad < 0 || (int64_t)bad[t] < *first_bad)) *first_bad = (int64_t)bad[t];
  for (size_t i = 0; i < nacc; i++) {
    rp::Sq sum = rp::q_small(0);
    for (int t = 0; t < threads; t++) rp::q_add(sum, sum, acc[t][i]);
    rp::q_to_le(shared + 32 * i, sum);
  }
  return BPMI_OK;
}

}  // extern "C"

// The same preparation on the GPU (rp_batch_kernels.hpp): the wire proofs are uploaded (in a few slices, so that the decoding of
// the points of slice c runs on the second lane while slice c + 1 is still on the link), one lane per proof and role parses,
// hashes and checks them, the weighted scalars are written straight into the caller's device scalar arrays, the proofs' points
// are decoded where they lie in the blobs into d_points, and only the (5 + 2n) shared coefficients and the verdict come back.
struct RpQueued { u32 *d_shared; unsigned long long *d_bad; u32 *d_fin; u32 ncols; };      // d_fin: room for the MSM scalars of the shared generators
// bpmi_rp_batch_group_values_dev: the preparation sums the cells per GROUP of `group` proofs instead of per batch and leaves one verdict
// byte per proof (k_rp_verdict, k_rp_group_colsum); the arrays live behind the preparation's own in ctx->rp_buf
struct RpGroups {
  u32 group, ngroups;        // in
  u32 *d_gsum, *d_gfin;      // out: ngroups x (5 + 2n) raw column sums; room for the ngroups x (3 + 2n) scalars of the groups' MSMs
  uint8_t *d_verdict, *d_ptflag;
  u32 *d_E, *d_vals;         // room for the window sums (37 per group) and the 64-byte values
  RpGroupRoute route; u32 W; // how the groups' MSMs run, with how many windows
};
// what the stages of one preparation share: the plan, the caller's arrays and the two device buffers the plan's offsets refer to
struct RpRun {
  const RpPlan &pl;
  const uint8_t *blobs, *weights, *seed;
  const uint64_t *blob_off;
  void *d_v_scalars, *d_pt_scalars, *d_points;
  RpGroups *G;               // nullptr: the batch as one
  char *din, *buf;           // ctx->stage_in, ctx->rp_buf (a class of a mixed batch: its own regions inside them)
  unsigned long long *bad = nullptr;      // a class of a mixed batch: the call's ONE bad word, set up by the caller, and ...
  uint64_t gbase = 0;                     // ... the global index of the class's proof 0 (rp_mixed_dev_host.hpp); nullptr / 0: a batch of its own
  u32 *d_contrib() const { return (u32 *)(buf + pl.contrib.off); }
  u32 *d_shared() const { return (u32 *)(buf + pl.shared.off); }
  unsigned long long *d_bad() const { return bad ? bad : (unsigned long long *)(buf + pl.o_bad); }
  u64 *d_T() const { return (u64 *)(buf + pl.T.off); }
  u32 *d_lens() const { return pl.v2 ? (u32 *)(buf + pl.lens.off) : nullptr; }
};
// A batch is read in the wire format of its FIRST proof.  A well-formed proof of the OTHER format inside it is not a forged proof: the
// device paths report it as an argument error ("mixed wire formats"), not as a verdict -- a verifier must be able to tell a
// sender's mix-up from an attack (the host path, bpmi_rp_batch_prepare, takes the formats proof by proof).
// cls: the class of a mixed batch the proof belongs to (first_bad counts inside it), named in the message; -1: a batch of its own.
static int rp_mixed_formats(bpmi_ctx *ctx, const uint8_t *blobs, uint64_t blobs_len, const uint64_t *blob_off, int64_t first_bad, int cls = -1) {
  if (first_bad < 0) return BPMI_OK;
  const uint64_t a0 = blob_off[0], a = blob_off[first_bad], e = blob_off[first_bad + 1];
  if (a0 + 5 > blobs_len || e > blobs_len || e < a + 5) return BPMI_OK;
  const uint8_t *b = blobs + a;
  const uint8_t call = (blobs[a0 + 4] == '2' || blobs[a0 + 4] == '3') ? blobs[a0 + 4] : (uint8_t)'1';
  if (!(b[0] == 'B' && b[1] == 'P' && b[2] == 'R' && b[3] == 'P' && b[4] >= '1' && b[4] <= '3' && b[4] != call)) return BPMI_OK;
  // WELL-FORMED in the format it claims?  (a format-1 proof whose magic a flipped bit turned into "BPRP3" is a bad proof, not a mix-up)
  const size_t len = (size_t)(e - a);
  rp::Parsed parsed;
  const bool well_formed = b[4] == '1' ? rp::parse_blob(parsed, b, len) : (len > 0 && rpw::v2_length(b, len) == len);
  if (well_formed)
    return fail(ctx, BPMI_E_ARG, "mixed wire formats: " + (cls < 0 ? std::string() : "class " + std::to_string(cls) + ", ") + "proof " + std::to_string(first_bad) +
                                     " is format " + std::string(1, (char)b[4]) + " in a format-" + std::string(1, (char)call) +
                                     " batch (one format per call; bpmi_rp_wire_v2_to_v1 converts)");
  return BPMI_OK;
}

// ---- the stages of rp_prepare_enqueue ------------------------------------------------------------------------------------------
// the buffers and events a preparation needs; R.din / R.buf are set
static int rp_ensure_sizes(bpmi_ctx *ctx, size_t stage_bytes, size_t pin_bytes, size_t need) {
  int rc = ensure_stage_in(ctx, stage_bytes);
  if (rc) return rc;
  rc = ensure_lane(ctx, 1);
  if (rc) return rc;
  rc = ensure_pin(ctx, pin_bytes);
  if (rc) return rc;
  for (int c = 0; c < RP_UPLOAD_SLICES; c++)
    if (!ctx->ev_slice[c]) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_slice[c], hipEventDisableTiming));
  if (need > ctx->rp_buf_bytes) {
    if (ctx->rp_buf) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(ctx->rp_buf)); ctx->rp_buf = nullptr; ctx->rp_buf_bytes = 0; }
    HIPCHK(ctx, hipMalloc(&ctx->rp_buf, need));
    ctx->rp_buf_bytes = need;
  }
  return BPMI_OK;
}
static int rp_ensure_buffers(bpmi_ctx *ctx, RpRun &R) {
  const int rc = rp_ensure_sizes(ctx, R.pl.stage_bytes, R.pl.pin_bytes, R.pl.need);
  if (rc) return rc;
  R.din = (char *)ctx->stage_in; R.buf = (char *)ctx->rp_buf;
  if (RpGroups *G = R.G) {
    char *b = R.buf;
    G->d_gsum = (u32 *)(b + R.pl.gsum.off); G->d_gfin = (u32 *)(b + R.pl.gfin.off); G->d_verdict = (uint8_t *)(b + R.pl.verdict.off);
    G->d_ptflag = (uint8_t *)(b + R.pl.ptflag.off); G->d_E = (u32 *)(b + R.pl.E.off); G->d_vals = (u32 *)(b + R.pl.vals.off);
    G->route = R.pl.route; G->W = R.pl.msm_windows;
  }
  return BPMI_OK;
}
// the points of the proofs [g0, g1), decoded where they lie in the uploaded blobs (it reads only the wire bytes)
static void rp_queue_decode(bpmi_ctx *ctx, const RpRun &R, hipStream_t st, u32 g0, u32 g1) {
  StageTimer t(ctx, ST_DECOMP, st);
  const u32 per = R.pl.per;
  const u64 npts = (u64)(g1 - g0) * per;
  hipLaunchKernelGGL(k_ec_decompress_wire, dim3((u32)((npts + 255) / 256)), dim3(256), 0, st, (const uint8_t *)R.din, (const u64 *)(R.din + R.pl.o_off) + g0,
                     R.pl.k, g1 - g0, R.gbase + g0, (u32)RP_MAX_PROOF_BYTES, (u32 *)R.d_points + 16ull * per * g0, R.d_bad(), R.G ? R.G->d_ptflag + g0 : (uint8_t *)nullptr);
}
// Offsets, weights, the cleared results, then the blobs in slices of whole proofs.  Under RP_DECODE_BESIDE the point decoding of a
// slice starts on the second lane as soon as the slice has arrived and runs beside the upload of the next one and, for the last
// slice, beside the preparation kernels.  ev_join: the second lane's work is in.
static int rp_queue_uploads(bpmi_ctx *ctx, const RpRun &R) {
  const RpPlan &pl = R.pl;
  const RpGroups *G = R.G;
  char *din = R.din;
  const size_t o_off = pl.o_off, o_w = pl.o_w, out_row = pl.out_row;
  const u32 P = pl.P, ncols = pl.ncols;
  const uint8_t *blobs = R.blobs, *weights = R.weights;
  const uint64_t *blob_off = R.blob_off;
  u32 *d_shared = R.d_shared();
  unsigned long long *d_bad = R.d_bad();
  HIPCHK(ctx, h2d(ctx, din + o_off, blob_off, 8 * ((size_t)P + 1), ctx->stream));
  if (weights) HIPCHK(ctx, h2d(ctx, din + o_w, weights, 128 * (size_t)P, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(d_shared, 0, out_row, ctx->stream));
  if (!R.bad) HIPCHK(ctx, hipMemsetAsync(d_bad, 0xFF, 8, ctx->stream));      // (a mixed batch's one word is cleared once, in front of its first class)
  if (G) {
    HIPCHK(ctx, hipMemsetAsync(G->d_gsum, 0, 32 * (size_t)ncols * G->ngroups, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(G->d_ptflag, 0, P, ctx->stream));            // (before the slices' events: the second lane's decoding sets flags)
  }
  for (u32 c = 0; c < pl.nsl; c++) {
    const u32 g0 = pl.sl[c].g0, g1 = pl.sl[c].g1;
    const uint64_t b0 = pl.sl[c].b0, b1 = pl.sl[c].b1;
    if (b1 > b0) HIPCHK(ctx, h2d(ctx, din + b0, blobs + b0, b1 - b0, ctx->stream));
    if (pl.decode == RP_DECODE_BESIDE) {
      HIPCHK(ctx, hipEventRecord(ctx->ev_slice[c], ctx->stream));
      HIPCHK(ctx, hipStreamWaitEvent(ctx->lane[1].stream, ctx->ev_slice[c], 0));
      rp_queue_decode(ctx, R, ctx->lane[1].stream, g0, g1);
    }
  }
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipEventRecord(ctx->ev_join, ctx->lane[1].stream));
  return BPMI_OK;
}
// the proofs as 8-byte words, word-major: format 1 transposed, formats 2 and 3 expanded to format 1 on the way
static int rp_queue_words(bpmi_ctx *ctx, const RpRun &R) {
  const RpPlan &pl = R.pl;
  const char *din = R.din;
  const u32 P = pl.P, W = pl.W;
  u64 *d_T = R.d_T();
  if (pl.v2) {
    // the expander writes the format-1 proofs word-major itself; what it does not write must read as zero
    const size_t T_bytes = pl.T.bytes;
    HIPCHK(ctx, hipMemsetAsync(d_T, 0, T_bytes, ctx->stream));
    StageTimer t(ctx, ST_RPPREP);
    hipLaunchKernelGGL(rpd::k_rp_expand_v2, dim3((P + 3) / 4), dim3(64), 0, ctx->stream, (const uint8_t *)din, (const u64 *)(din + pl.o_off), P, pl.k, W, d_T, R.d_lens(),
                       (u32)pl.fmt0, pl.rp_prio);
  } else {
    StageTimer t(ctx, ST_RPPREP);
    hipLaunchKernelGGL(rpd::k_rp_transpose, dim3((P + 63) / 64, (W + 63) / 64), dim3(256), 0, ctx->stream, (const uint8_t *)din, (const u64 *)(din + pl.o_off), P, W, d_T);
  }
  return BPMI_OK;
}
// group mode, behind the roles and elements of the proofs [base, base + cnt): one verdict byte per proof, then the cells of the
// unflagged proofs summed per group
static int rp_queue_group_rows(bpmi_ctx *ctx, const RpRun &R, u32 base, u32 cnt) {
  const RpPlan &pl = R.pl;
  const RpGroups *G = R.G;
  if (base == 0 && pl.decode == RP_DECODE_BESIDE) HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));      // the two lanes join: every point flag is set
  StageTimer t(ctx, ST_RPELEM);
  rpd::VerdictArgs va;
  va.role_status = (const uint8_t *)(R.din + pl.o_st); va.pt_flag = G->d_ptflag; va.verdict = G->d_verdict;
  va.Pall = pl.P; va.first = base; va.cnt = cnt; va.m = pl.m; va.per = pl.per; va.only_role = ctx->opt_rp_only_role;
  va.v_scalars = (u32 *)R.d_v_scalars; va.pt_scalars = (u32 *)R.d_pt_scalars; va.points = (u32 *)R.d_points;
  hipLaunchKernelGGL(rpd::k_rp_verdict, dim3((u32)(((uint64_t)cnt * (pl.m + pl.per) + 255) / 256)), dim3(256), 0, ctx->stream, va);
  const RpGroupChunk gc = rp_group_chunk(G->group, base, cnt);
  hipLaunchKernelGGL(rpd::k_rp_group_colsum, dim3(pl.ncols * gc.nblk), dim3(64), 0, ctx->stream, (const u32 *)R.d_contrib(), cnt, base, (const uint8_t *)G->d_verdict,
                     G->group, gc.t0, gc.nt, gc.lpg, pl.ncols, G->d_gsum);
  return BPMI_OK;
}
// the kernels' parameters: what every row chunk of a preparation shares, then what the chunk of the proofs [base, base + cnt) adds
static rpd::Params rp_params(bpmi_ctx *ctx, const RpRun &R, uint32_t n_gens) {
  const RpPlan &pl = R.pl;
  const uint8_t *seed = R.seed;
  rpd::Params q;
  memset(&q, 0, sizeof(q));
  q.Tstride = pl.P;
  q.weights = R.weights ? (const uint8_t *)(R.din + pl.o_w) : nullptr;
  for (int i = 0; i < 8; i++) q.seed[i] = seed ? ((u32)seed[4 * i] << 24) | ((u32)seed[4 * i + 1] << 16) | ((u32)seed[4 * i + 2] << 8) | seed[4 * i + 3] : 0;
  q.n = n_gens; q.k = pl.k; q.m = pl.m; q.Pall = pl.P; q.only_role = ctx->opt_rp_only_role;
  q.contrib = R.d_contrib();
  q.prio = pl.rp_prio;
  q.ctx = (u32 *)(R.buf + pl.ctx.off);
  q.bad = R.d_bad();
  q.gbase = R.gbase;
  q.lanes = pl.lanes;
  return q;
}
static void rp_params_rows(rpd::Params &q, const RpRun &R, u32 base, u32 cnt) {
  const RpPlan &pl = R.pl;
  q.off = (const u64 *)(R.din + pl.o_off) + base;
  q.lens = pl.v2 ? R.d_lens() + base : nullptr;
  q.T = R.d_T() + base;
  q.P = cnt; q.first = base;
  q.v_scalars = (u32 *)R.d_v_scalars + 8 * (size_t)base * pl.m;
  q.pt_scalars = (u32 *)R.d_pt_scalars + 8 * (size_t)base * pl.per;
  q.status = (uint8_t *)(R.din + pl.o_st) + base;
}
// rows of at most pl.rows proofs: roles, elements, then the column sums of the batch or of its groups
static int rp_queue_rows(bpmi_ctx *ctx, const RpRun &R, uint32_t n_gens) {
  const RpPlan &pl = R.pl;
  const u32 P = pl.P, lanes = pl.lanes;
  u32 *d_contrib = R.d_contrib();
  rpd::Params q = rp_params(ctx, R, n_gens);
  rpd::ElemGeom eg;
  eg.el_log = pl.el_log;
  eg.ranges = pl.ranges;
  for (u32 base = 0; base < P; base += pl.rows) {
    const u32 cnt = std::min(pl.rows, P - base);
    rp_params_rows(q, R, base, cnt);
    {
      StageTimer t(ctx, ST_RPPREP);
      hipLaunchKernelGGL(rpd::k_rp_roles, dim3(RP_ROLES * ((cnt + lanes - 1) / lanes)), dim3(64), pl.lds_bytes, ctx->stream, q);
    }
    {
      StageTimer t(ctx, ST_RPELEM);
      hipLaunchKernelGGL(rpd::k_rp_elements, dim3(2 * eg.ranges * ((cnt + 63) / 64)), dim3(64), 0, ctx->stream, q, eg);
      if (!R.G) hipLaunchKernelGGL(rpd::k_rp_colsum, dim3(pl.ncols), dim3(256), 0, ctx->stream, (const u32 *)d_contrib, cnt, R.d_shared());
    }
    if (R.G) { const int rc = rp_queue_group_rows(ctx, R, base, cnt); if (rc) return rc; }
  }
  return BPMI_OK;
}
// queues everything on the ctx's two lanes and returns without waiting; the results stay on the device (d_shared: 5 + 2n
// scalars of 8 words, *d_bad behind them).  The caller waits for both lanes whatever this returns.
// Where the points are decoded (pl.decode, rp_batch_plan_host.hpp):
//   RP_DECODE_BESIDE  option rp_overlap = 1, the default: slice by slice on the second lane (rp_queue_uploads); the lanes join at the
//                     end, in group mode in front of the first k_rp_verdict (rp_queue_group_rows), which reads the point flags
//   RP_DECODE_LAST    rp_overlap = 0 (measurements only), the batch as one: one launch BEHIND the preparation kernels on the same
//                     stream, so that every kernel's duration is its own
//   RP_DECODE_FIRST   rp_overlap = 0, group mode: one launch in FRONT of the rows -- the per-proof verdict needs the point flags
static int rp_prepare_enqueue(bpmi_ctx *ctx, uint32_t n_gens, uint32_t m, uint64_t n_proofs, const uint8_t *blobs, uint64_t blobs_len, const uint64_t *blob_off,
                              const uint8_t *weights, const uint8_t *seed, void *d_v_scalars, void *d_pt_scalars, void *d_points, RpQueued &Q,
                              RpGroups *G = nullptr) {
  const RpPlan pl = rp_prepare_plan(*ctx, n_gens, m, n_proofs, blobs, blobs_len, blob_off, weights != nullptr, G ? G->group : 0);
  if (pl.err) return fail(ctx, pl.err, pl.msg);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  RpRun R{pl, blobs, weights, seed, blob_off, d_v_scalars, d_pt_scalars, d_points, G, nullptr, nullptr};
  int rc = rp_ensure_buffers(ctx, R);
  if (rc) return rc;
  Q.d_shared = R.d_shared(); Q.d_bad = R.d_bad(); Q.d_fin = (u32 *)(R.buf + pl.o_fin); Q.ncols = pl.ncols;
  rc = rp_queue_uploads(ctx, R);
  if (rc) return rc;
  rc = rp_queue_words(ctx, R);
  if (rc) return rc;
  if (pl.decode == RP_DECODE_FIRST) rp_queue_decode(ctx, R, ctx->stream, 0, pl.P);
  rc = rp_queue_rows(ctx, R, n_gens);
  if (rc) return rc;
  if (pl.decode == RP_DECODE_LAST) rp_queue_decode(ctx, R, ctx->stream, 0, pl.P);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
  return BPMI_OK;
}
// both lanes idle again; the first error of (rc, the two waits)
static int rp_wait_lanes(bpmi_ctx *ctx, int rc) {
  const hipError_t e0 = wait_stream(ctx, ctx->stream), e1 = ctx->lane[1].stream ? wait_stream(ctx, ctx->lane[1].stream) : hipSuccess;      // (lane 2 never takes part in a batch)
  if (rc) return rc;
  HIPCHK(ctx, e0);
  HIPCHK(ctx, e1);
  return BPMI_OK;
}

// ---- what the entry points share -------------------------------------------------------------------------------------------------
// the sizes of the batch's one MSM over [shared generators | commitments | proof points], and its limit
struct RpBatchDims { u32 k, per, nshared; uint64_t nv, npts; };
static int rp_batch_dims(bpmi_ctx *ctx, uint32_t n_gens, uint32_t m, uint64_t n_proofs, RpBatchDims &d) {
  (void)log2_exact(n_gens, d.k);
  d.per = 6 + 2 * d.k; d.nshared = 3 + 2 * n_gens;
  d.nv = n_proofs * m; d.npts = n_proofs * d.per;
  if (3 + 2 * (uint64_t)n_gens + d.nv + d.npts > (1ull << 23)) return fail(ctx, BPMI_E_ARG, "at most 2^23 points in the batch's MSM");
  return BPMI_OK;
}
// commitments: the first nv points / scalars of the per-proof arrays; their on-curve check (and the generators', from validate = 2)
// is queued behind the upload, in the caller's PointCheck: the caller reads pc.verdict() after its last wait
static int rp_upload_commitments(bpmi_ctx *ctx, const uint8_t *v_points, void *d_points, const void *d_gens, const RpBatchDims &d, PointCheck &pc) {
  HIPCHK(ctx, h2d(ctx, d_points, v_points, 64 * d.nv, ctx->stream));
  pc.queue(d_points, d.nv, "v_points");
  if (ctx->opt_validate >= 2) pc.queue(d_gens, d.nshared, "d_gens");
  return pc.fetch();
}
// the index k_rp_roles and the decoding left at p (~0: none)
static int64_t rp_first_bad_at(const void *p) {
  unsigned long long bad;
  memcpy(&bad, p, 8);
  return bad == ~0ull ? -1 : (int64_t)bad;
}
// The ending of a call: a flagged proof that is a well-formed proof of another format is an argument error, and a profiling run
// that checked part of every proof must never read as "all valid"
static int rp_finish_verdict(bpmi_ctx *ctx, const uint8_t *blobs, uint64_t blobs_len, const uint64_t *blob_off, int64_t *first_bad) {
  const int rc = rp_mixed_formats(ctx, blobs, blobs_len, blob_off, *first_bad);
  if (rc) return rc;
  if (ctx->opt_rp_only_role >= 0) *first_bad = 0;
  return BPMI_OK;
}

extern "C" {

int bpmi_rp_batch_prepare_dev(bpmi_ctx *ctx, uint32_t n_gens, uint32_t values_per_proof, uint64_t n_proofs, const uint8_t *blobs, uint64_t blobs_len,
                              const uint64_t *blob_off, const uint8_t *weights, const uint8_t *seed, void *d_v_scalars, void *d_pt_scalars, void *d_points,
                              uint8_t *shared, int64_t *first_bad) {
  if (!ctx) return BPMI_E_ARG;
  if (!blobs || !blob_off || (!weights && !seed) || !d_v_scalars || !d_pt_scalars || !d_points || !shared || !first_bad) return fail(ctx, BPMI_E_ARG, "null argument");
  *first_bad = -1;
  RpQueued Q;
  int rc = rp_prepare_enqueue(ctx, n_gens, values_per_proof, n_proofs, blobs, blobs_len, blob_off, weights, seed, d_v_scalars, d_pt_scalars, d_points, Q);
  const size_t out_row = rc ? 0 : 32 * (size_t)Q.ncols;
  if (!rc && hipMemcpyAsync(ctx->pin, Q.d_shared, out_row + 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = fail(ctx, BPMI_E_HIP, "copy of the shared coefficients failed");
  // an error in the middle must not return while the second lane is still writing into the caller's point array
  rc = rp_wait_lanes(ctx, rc);
  if (rc) return rc;
  memcpy(shared, ctx->pin, out_row);
  *first_bad = rp_first_bad_at((char *)ctx->pin + out_row);
  return rp_finish_verdict(ctx, blobs, blobs_len, blob_off, first_bad);
}

// The whole batch verification in ONE call: preparation as above, the shared coefficients folded on the device into the scalars of
// the 3 + 2n shared generators (k_rp_shared_scalars), and the batch's one MSM over [shared generators | commitments | proof
// points] -- no host round trip between the preparation and the MSM.  out = the 64-byte value of the combination (the identity
// for a valid batch; a sharded caller folds the ranks' values), *first_bad as above (then `out` means nothing).
//   v_points  HOST, n_proofs x values_per_proof x 64 B: the commitments, in proof order
//   d_gens    DEVICE, (3 + 2 n_gens) x 64 B: g, h, u, gs, hs (uploaded once per verifier)
//   d_points  DEVICE scratch, (n_proofs (values_per_proof + 6 + 2k)) x 64 B;  d_scalars  DEVICE scratch, the same count x 32 B
int bpmi_rp_batch_verify_dev(bpmi_ctx *ctx, uint32_t n_gens, uint32_t values_per_proof, uint64_t n_proofs, const uint8_t *blobs, uint64_t blobs_len,
                             const uint64_t *blob_off, const uint8_t *weights, const uint8_t *seed, const uint8_t *v_points, const void *d_gens, void *d_points,
                             void *d_scalars, uint8_t out[64], int64_t *first_bad) {
  if (!ctx) return BPMI_E_ARG;
  if (!blobs || !blob_off || (!weights && !seed) || !v_points || !d_gens || !d_points || !d_scalars || !out || !first_bad) return fail(ctx, BPMI_E_ARG, "null argument");
  *first_bad = -1;
  RpBatchDims d;
  int rc = rp_batch_dims(ctx, n_gens, values_per_proof, n_proofs, d);
  if (rc) return rc;
  const uint64_t nv = d.nv, npts = d.npts;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  PointCheck pc(ctx, "bpmi_rp_batch_verify_dev", ctx->stream, ctx->opt_validate >= 1);
  rc = rp_upload_commitments(ctx, v_points, d_points, d_gens, d, pc);
  if (rc) return rc;
  RpQueued Q;
  rc = rp_prepare_enqueue(ctx, n_gens, values_per_proof, n_proofs, blobs, blobs_len, blob_off, weights, seed, d_scalars, (char *)d_scalars + 32 * nv,
                          (char *)d_points + 64 * nv, Q);
  if (!rc) {
    // scalars of g, h, u, gs_i, hs_i: c_g, c_h, c_u, c_gs[i] + gs_const, c_hs[i] + hs_const -- in place behind the raw sums
    {
      StageTimer t(ctx, ST_RPELEM);
      hipLaunchKernelGGL(rpd::k_rp_shared_scalars, dim3((3 + 2 * n_gens + 255) / 256), dim3(256), 0, ctx->stream, (const u32 *)Q.d_shared, n_gens, Q.d_fin);
    }
    if (hipMemcpyAsync(ctx->pin, Q.d_bad, 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = fail(ctx, BPMI_E_HIP, "copy of the verdict failed");
  }
  if (rc) return rp_wait_lanes(ctx, rc);
  Segs s = segs_init();
  s.pts[0] = (const u32 *)d_gens; s.sc[0] = Q.d_fin; s.n[0] = 3 + 2 * n_gens;
  s.pts[1] = (const u32 *)d_points; s.sc[1] = (const u32 *)d_scalars; s.n[1] = (u32)(nv + npts);
  s.total = s.n[0] + s.n[1];
  rc = msm_run(ctx, s, out);                      // waits for the MSM (ctx stream: behind everything queued above)
  rc = rp_wait_lanes(ctx, rc);
  if (rc) return rc;
  rc = pc.verdict();
  if (rc) { memset(out, 0xFF, 64); return rc; }                    // (never the identity)
  *first_bad = rp_first_bad_at(ctx->pin);
  rc = rp_finish_verdict(ctx, blobs, blobs_len, blob_off, first_bad);
  if (rc) memset(out, 0xFF, 64);
  return rc;
}

}  // extern "C"

// The groups' MSMs over [shared generators | the group's commitments | the group's proof points] as ONE launch over (group, window)
// (k_msm_group) with a device tail (k_group_tail); the values are copied to ctx->pin
static int rp_queue_group_msms(bpmi_ctx *ctx, const RpGroups &G, const RpBatchDims &d, uint32_t m, uint64_t n_proofs, const void *d_gens, const void *d_points,
                               const void *d_scalars) {
  const uint64_t nv = d.nv;
  const u32 W = G.W;
  const size_t vals_bytes = 64 * (size_t)G.ngroups;
  GroupMsm J;
  J.gens = (const u32 *)d_gens; J.gsc = G.d_gfin;
  J.v_pts = (const u32 *)d_points; J.v_sc = (const u32 *)d_scalars;
  J.p_pts = (const u32 *)d_points + 16 * nv; J.p_sc = (const u32 *)d_scalars + 8 * nv;
  J.nshared = d.nshared; J.m = m; J.per = d.per; J.group = G.group; J.P = (u32)n_proofs; J.W = W; J.E = G.d_E;
  {
    StageTimer t(ctx, ST_ACCUM);
    group_msm_launch(ctx, G.route == RP_GROUPS_LIGHT, k_msm_group<GROUP_LIGHT_THREADS, GROUP_LIGHT_NMAX>, k_msm_group<MID_THREADS, MID_NMAX>, G.ngroups, W, J);
    group_tail_launch(ctx, G.d_E, W, G.ngroups, G.d_vals);                         // (both: ipa_verify_msm_host.hpp)
  }
  if (hipGetLastError() != hipSuccess) return fail(ctx, BPMI_E_HIP, "launch of the group MSMs failed");
  if (hipMemcpyAsync(ctx->pin, G.d_vals, vals_bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) return fail(ctx, BPMI_E_HIP, "copy of the group values failed");
  return BPMI_OK;
}
// groups beyond the one-launch kernel's capacity: one MSM each on the three segments
static int rp_run_group_msms(bpmi_ctx *ctx, const RpGroups &G, const RpBatchDims &d, uint32_t m, uint64_t n_proofs, const void *d_gens, const void *d_points,
                             const void *d_scalars, uint8_t *values) {
  const uint64_t nv = d.nv;
  const u32 per = d.per, nshared = d.nshared;
  int rc = BPMI_OK;
  for (u32 t = 0; t < G.ngroups && !rc; t++) {
    const uint64_t g0 = (uint64_t)t * G.group, cnt = std::min<uint64_t>(G.group, n_proofs - g0);
    Segs s = segs_init();
    s.pts[0] = (const u32 *)d_gens; s.sc[0] = G.d_gfin + 8 * (size_t)nshared * t; s.n[0] = nshared;
    s.pts[1] = (const u32 *)d_points + 16 * m * g0; s.sc[1] = (const u32 *)d_scalars + 8 * m * g0; s.n[1] = (u32)(cnt * m);
    s.pts[2] = (const u32 *)d_points + 16 * (nv + per * g0); s.sc[2] = (const u32 *)d_scalars + 8 * (nv + per * g0); s.n[2] = (u32)(cnt * per);
    s.total = s.n[0] + s.n[1] + s.n[2];
    rc = msm_run(ctx, s, values + 64 * (size_t)t);
  }
  return rp_wait_lanes(ctx, rc);
}

extern "C" {

// Which proofs of a rejected batch are the bad ones (replaces what a caller of the reference gets from verifying one proof at a time:
// src/rangeproofs/rangeproof_verifier.py:55-99, rangeproof_aggreg_verifier.py:55-108): the preparation of bpmi_rp_batch_verify_dev, but the
// cells are summed per GROUP of `group` consecutive proofs, the groups' MSMs over [shared generators | the group's commitments | the
// group's proof points] run as ONE launch over (group, window) (k_msm_group) with a device tail (k_group_tail), and every proof gets a
// verdict byte for its byte-level checks.  values[t] = the 64-byte value of group t's combination over its UNFLAGGED proofs (64 zero
// bytes: all of them verify); status[i] = bit 0: a byte-level check failed (parse, transcript, scalar range) | bit 1: an invalid point
// encoding.  A flagged proof contributes to no group.  A group whose MSM does not fit the one-launch kernel (3 + 2n + group (m + 6 + 2k) >
// MID_NMAX pairs) goes through msm_run, group by group: the same 64 bytes.
int bpmi_rp_batch_group_values_dev(bpmi_ctx *ctx, uint32_t n_gens, uint32_t values_per_proof, uint64_t n_proofs, const uint8_t *blobs, uint64_t blobs_len,
                                   const uint64_t *blob_off, const uint8_t *weights, const uint8_t *seed, const uint8_t *v_points, const void *d_gens,
                                   void *d_points, void *d_scalars, uint64_t group, uint8_t *values, uint8_t *status) {
  if (!ctx) return BPMI_E_ARG;
  if (!blobs || !blob_off || (!weights && !seed) || !v_points || !d_gens || !d_points || !d_scalars || !values || !status) return fail(ctx, BPMI_E_ARG, "null argument");
  if (group < 1) return fail(ctx, BPMI_E_ARG, "group must be at least 1");
  if (n_proofs == 0 || n_proofs > (1ull << 22)) return fail(ctx, BPMI_E_ARG, "n_proofs must be in [1, 2^22]");
  const uint32_t m = values_per_proof;
  RpBatchDims d;
  int rc = rp_batch_dims(ctx, n_gens, m, n_proofs, d);
  if (rc) return rc;
  const uint64_t nv = d.nv;
  RpGroups G;
  memset(&G, 0, sizeof(G));
  const RpGroupShape gs = rp_group_shape(group, n_proofs);
  G.group = gs.group; G.ngroups = gs.ngroups;
  if ((uint64_t)G.ngroups * d.nshared > (1ull << 26)) return fail(ctx, BPMI_E_ARG, "too many groups: n_groups x (3 + 2 n_gens) must not exceed 2^26");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t vals_bytes = 64 * (size_t)G.ngroups;
  rc = ensure_pin(ctx, std::max<size_t>(32 * (size_t)(5 + 2 * n_gens) + 64, vals_bytes + n_proofs + 64));
  if (rc) return rc;
  PointCheck pc(ctx, "bpmi_rp_batch_group_values_dev", ctx->stream, ctx->opt_validate >= 1);
  rc = rp_upload_commitments(ctx, v_points, d_points, d_gens, d, pc);
  if (rc) return rc;
  RpQueued Q;
  rc = rp_prepare_enqueue(ctx, n_gens, m, n_proofs, blobs, blobs_len, blob_off, weights, seed, d_scalars, (char *)d_scalars + 32 * nv, (char *)d_points + 64 * nv, Q, &G);
  if (rc) return rp_wait_lanes(ctx, rc);
  {
    StageTimer t(ctx, ST_RPELEM);
    hipLaunchKernelGGL(rpd::k_rp_group_scalars, dim3((u32)(((uint64_t)G.ngroups * d.nshared + 255) / 256)), dim3(256), 0, ctx->stream, (const u32 *)G.d_gsum, n_gens,
                       G.ngroups, G.d_gfin);
  }
  if (G.route != RP_GROUPS_MSM_RUN) rc = rp_queue_group_msms(ctx, G, d, m, n_proofs, d_gens, d_points, d_scalars);
  if (!rc && hipMemcpyAsync((char *)ctx->pin + vals_bytes, G.d_verdict, n_proofs, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
    rc = fail(ctx, BPMI_E_HIP, "copy of the verdicts failed");
  rc = rp_wait_lanes(ctx, rc);
  if (rc) return rc;
  memcpy(status, (char *)ctx->pin + vals_bytes, n_proofs);
  if (G.route != RP_GROUPS_MSM_RUN) {
    memcpy(values, ctx->pin, vals_bytes);
  } else {
    rc = rp_run_group_msms(ctx, G, d, m, n_proofs, d_gens, d_points, d_scalars, values);
    if (rc) { memset(values, 0xFF, vals_bytes); return rc; }
  }
  rc = pc.verdict();
  if (rc) { memset(values, 0xFF, vals_bytes); return rc; }
  int64_t first_flagged = -1;
  for (uint64_t i = 0; i < n_proofs && first_flagged < 0; i++) if (status[i]) first_flagged = (int64_t)i;
  rc = rp_mixed_formats(ctx, blobs, blobs_len, blob_off, first_flagged);
  if (rc) { memset(values, 0xFF, vals_bytes); return rc; }
  return BPMI_OK;
}

}  // extern "C"
