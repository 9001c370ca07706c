// ipa_wire_dev_host.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).  HOST code.
// Inner-product proofs in the wire format BPIP2 behind the C ABI: bpmi_ipa_wire_bytes, bpmi_ipa_wire_encode and bpmi_ipa_wire_expand
// (host code, ipa_wire_host.hpp), bpmi_ipa_wire_expand_dev (the same bytes by the kernels of ipa_wire_kernels.hpp, downloaded: the
// comparison hook) and bpmi_ipa_verify_batch_wire_dev: the blobs are uploaded as they are, decompressed and expanded in device
// memory, and the kernel part of the packed verifier (ipap_launch_kernels, ipa_packed_dev_host.hpp) runs over the regions the
// expander filled -- then ipab_svector_launches and the one MSM, as bpmi_ipa_verify_batch_packed_dev.  Plan and argument errors:
// ipa_wire_plan_host.hpp.  Protocol 2 only.
#pragma once

// what the expansion of a call needs on the device: the blobs and their offsets uploaded, the flags zeroed
struct IpawDev {
  const IpawPlan &pl;
  char *base;
  uint64_t origin;                   // the host's off[0]
  const uint8_t *blobs() const { return (const uint8_t *)base + pl.o_wire; }
  const u64 *off() const { return (const u64 *)(base + pl.o_off); }
  u32 *lens() const { return (u32 *)(base + pl.o_lens); }
  uint8_t *badflag() const { return (uint8_t *)base + pl.o_flags; }
  uint8_t *ptflag() const { return (uint8_t *)base + pl.o_flags + pl.n_proofs; }
};
static int ipaw_upload(bpmi_ctx *ctx, const IpawPlan &pl, const IpaWireIn &in) {
  char *base = (char *)ctx->stage_in;
  if (pl.wire_bytes) HIPCHK(ctx, h2d(ctx, base + pl.o_wire, in.blobs + in.off[0], pl.wire_bytes, ctx->stream));
  HIPCHK(ctx, h2d(ctx, base + pl.o_off, in.off, pl.b_off, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(base + pl.o_flags, 0, pl.b_flags, ctx->stream));
  return BPMI_OK;
}
// every proof's points into the LR region (one launch for the call: the rows do not depend on the launches of T)
static void ipaw_decompress_launch(bpmi_ctx *ctx, const IpawDev &d) {
  const IpawPlan &pl = d.pl;
  if (!pl.k) return;
  StageTimer t(ctx, ST_DECOMP);
  const uint64_t npts = 2ull * pl.k * pl.n_proofs;
  hipLaunchKernelGGL(ipad::k_ipaw_decompress, dim3((u32)((npts + 255) / 256)), dim3(256), 0, ctx->stream, d.blobs(), d.off(), d.origin, pl.k, (u64)0, (u32)pl.n_proofs,
                     (u32 *)(d.base + pl.o_lr), d.ptflag());
}
// proofs [first, first + cnt): T zeroed (the expander ORs the shared words in), the expansion, the offsets of the launch's proofs.
// Timed as "rp_elements": no other kernel of an inner-product call reports under that stage
static void ipaw_expand_launch(bpmi_ctx *ctx, const IpawDev &d, uint64_t first, u32 cnt) {
  const IpawPlan &pl = d.pl;
  StageTimer t(ctx, ST_RPELEM);
  (void)hipMemsetAsync(d.base + pl.o_T, 0, 8ull * pl.W * cnt, ctx->stream);
  hipLaunchKernelGGL(ipad::k_ipaw_expand, dim3((cnt + 3) / 4), dim3(64), 0, ctx->stream, d.blobs(), d.off(), d.origin, pl.k, (u64)first, cnt, pl.W, (u64 *)(d.base + pl.o_T),
                     (u32 *)(d.base + pl.o_ab), (u32 *)(d.base + pl.o_xs), (u32 *)(d.base + pl.o_start), d.lens(), d.badflag());
  hipLaunchKernelGGL(ipad::k_ipaw_offsets, dim3(1), dim3(256), 0, ctx->stream, (const u32 *)d.lens(), (u64 *)(d.base + pl.o_troff), (u64)first, cnt);
}

extern "C" {

uint64_t bpmi_ipa_wire_bytes(uint32_t k, uint64_t prefix_len) { return ipaw_wire_bytes(k, prefix_len); }

int bpmi_ipa_wire_encode(uint32_t k, int protocol, uint64_t n_proofs, const uint8_t *ab, const uint8_t *xs, const uint8_t *LR, const uint8_t *transcripts, const uint64_t *tr_off,
                         const uint32_t *start, uint8_t *blobs, uint64_t cap, uint64_t *off, uint8_t *status) {
  static const std::string fn = "bpmi_ipa_wire_encode: ";
  if (protocol != 2) return fail(nullptr, BPMI_E_ARG, fn + "the wire format holds Protocol-2 proofs only");
  if (k > IPAB_K_MAX) return fail(nullptr, BPMI_E_ARG, fn + "n must be 2^k, k <= 22");
  if (!off) return fail(nullptr, BPMI_E_ARG, fn + "null argument");
  off[0] = 0;
  if (n_proofs == 0) return BPMI_OK;
  if (!ab || !transcripts || !tr_off || !blobs || !status || (k && (!xs || !LR))) return fail(nullptr, BPMI_E_ARG, fn + "null argument (xs and LR may be NULL only at k = 0)");
  for (uint64_t p = 0; p < n_proofs; p++)
    if (tr_off[p + 1] < tr_off[p]) return fail(nullptr, BPMI_E_ARG, fn + "tr_off must not decrease");
  try {
    if (!ipaw::encode_all(k, n_proofs, ab, xs, LR, transcripts, tr_off, start, blobs, cap, off, status))
      return fail(nullptr, BPMI_E_ARG, fn + "cap is too small (n_proofs x (78 + 98 k) + the transcripts' bytes always suffice)");
  } catch (const std::exception &) {
    return fail(nullptr, BPMI_E_NOMEM, fn + "out of host memory");
  }
  return BPMI_OK;
}

int bpmi_ipa_wire_expand(uint32_t k, int protocol, uint64_t n_proofs, const uint8_t *blobs, const uint64_t *off, uint8_t *ab, uint8_t *xs, uint8_t *LR, uint8_t *transcripts,
                         uint64_t cap, uint64_t *tr_off, uint32_t *start, uint8_t *status) {
  static const std::string fn = "bpmi_ipa_wire_expand: ";
  if (protocol != 2) return fail(nullptr, BPMI_E_ARG, fn + "the wire format holds Protocol-2 proofs only");
  if (n_proofs == 0) { if (tr_off) tr_off[0] = 0; return BPMI_OK; }
  IpaWireIn in;
  in.blobs = blobs; in.off = off;
  const IpawPlan pl = ipa_wire_plan(BpmiOptions(), k, protocol, n_proofs, in, false, 0, 0);
  if (pl.err) return fail(nullptr, pl.err, fn + pl.msg);
  if (!ab || !transcripts || !tr_off || !start || !status || (k && (!xs || !LR))) return fail(nullptr, BPMI_E_ARG, fn + "null argument (xs and LR may be NULL only at k = 0)");
  if (cap < pl.text_bound) return fail(nullptr, BPMI_E_ARG, fn + "cap is below the expansion bound (per proof: its prefix + 169 k bytes)");
  try {
    ipaw::expand_all(k, n_proofs, blobs, off, ab, xs, LR, transcripts, tr_off, start, status);
  } catch (const std::exception &) {
    return fail(nullptr, BPMI_E_NOMEM, fn + "out of host memory");
  }
  return BPMI_OK;
}

int bpmi_ipa_wire_expand_dev(bpmi_ctx *ctx, uint32_t k, int protocol, uint64_t n_proofs, const uint8_t *blobs, const uint64_t *off, uint8_t *ab, uint8_t *xs, uint8_t *LR,
                             uint8_t *transcripts, uint64_t cap, uint64_t *tr_off, uint32_t *start, uint8_t *status) {
  static const char *const fn = "bpmi_ipa_wire_expand_dev";
  if (!ctx) return BPMI_E_ARG;
  if (protocol != 2) return fail(ctx, BPMI_E_ARG, std::string(fn) + ": the wire format holds Protocol-2 proofs only");
  if (n_proofs == 0) { if (tr_off) tr_off[0] = 0; return BPMI_OK; }
  IpaWireIn in;
  in.blobs = blobs; in.off = off;
  const IpawPlan pl = ipa_wire_plan(*ctx, k, protocol, n_proofs, in, false, 0, ctx->ipap_t_budget);
  if (pl.err) return fail(ctx, pl.err, std::string(fn) + ": " + pl.msg);
  if (!ab || !transcripts || !tr_off || !start || !status || (k && (!xs || !LR))) return fail(ctx, BPMI_E_ARG, std::string(fn) + ": null argument (xs and LR may be NULL only at k = 0)");
  if (cap < pl.text_bound) return fail(ctx, BPMI_E_ARG, std::string(fn) + ": cap is below the expansion bound (per proof: its prefix + 169 k bytes)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = ensure_stage_in(ctx, pl.total_bytes + 512);
  if (rc) return rc;
  rc = ipaw_upload(ctx, pl, in);
  if (rc) return rc;
  const IpawDev d = {pl, (char *)ctx->stage_in, off[0]};
  hipStream_t st = ctx->stream;
  ipaw_decompress_launch(ctx, d);
  try {
    // the transcripts come back launch by launch, word-major as the roles read them, and are put in proof order here
    std::vector<u64> T((size_t)pl.W * pl.rows);
    std::vector<u32> lens(n_proofs);
    uint64_t at = 0;
    tr_off[0] = 0;
    for (uint64_t first = 0; first < n_proofs; first += pl.rows) {
      const u32 cnt = (u32)(n_proofs - first < pl.rows ? n_proofs - first : pl.rows);
      ipaw_expand_launch(ctx, d, first, cnt);
      HIPCHK(ctx, hipGetLastError());
      HIPCHK(ctx, hipMemcpyAsync(T.data(), d.base + pl.o_T, 8ull * pl.W * cnt, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipMemcpyAsync(lens.data() + first, d.lens() + first, 4ull * cnt, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      for (u32 r = 0; r < cnt; r++) {
        const u32 len = lens[first + r];
        if (len > IPAP_MAX_TRANSCRIPT || at + len > cap) return fail(ctx, BPMI_E_STATE, std::string(fn) + ": an expansion longer than its bound");
        for (u32 o = 0; o < len; o += 8) {
          const u64 word = T[(size_t)(o / 8) * cnt + r];
          memcpy(transcripts + at + o, &word, len - o < 8 ? len - o : 8);
        }
        at += len;
      }
    }
  } catch (const std::bad_alloc &) {
    return fail(ctx, BPMI_E_NOMEM, std::string(fn) + ": out of host memory");
  }
  std::vector<uint8_t> flags(2 * n_proofs);
  HIPCHK(ctx, hipMemcpyAsync(ab, d.base + pl.o_ab, pl.b_ab, hipMemcpyDeviceToHost, st));
  if (k) {
    HIPCHK(ctx, hipMemcpyAsync(xs, d.base + pl.o_xs, pl.b_xs, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(LR, d.base + pl.o_lr, pl.b_lr, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(ctx, hipMemcpyAsync(tr_off, d.base + pl.o_troff, pl.b_troff, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(start, d.base + pl.o_start, pl.b_start, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(flags.data(), d.base + pl.o_flags, pl.b_flags, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  for (uint64_t p = 0; p < n_proofs; p++) status[p] = (uint8_t)((flags[p] ? 1 : 0) | (flags[n_proofs + p] ? 2 : 0));
  return BPMI_OK;
}

int bpmi_ipa_verify_batch_wire_dev(bpmi_ctx *ctx, const void *d_g, const void *d_h, const void *d_hscale, uint64_t n, int protocol, uint64_t n_proofs, const uint8_t *blobs,
                                   const uint64_t *off, const uint8_t *u, const uint8_t *P, const uint8_t *weights, const uint8_t *seed, uint8_t out[64],
                                   uint8_t *status) {
  static const char *const fn = "bpmi_ipa_verify_batch_wire_dev";
  if (!ctx) return BPMI_E_ARG;
  if (!out) return fail(ctx, BPMI_E_ARG, std::string(fn) + ": null argument");
  if (protocol != 2) return fail(ctx, BPMI_E_ARG, std::string(fn) + ": the wire format holds Protocol-2 proofs only");
  if (n_proofs == 0) { memset(out, 0, 64); return BPMI_OK; }
  if (!d_g || !d_h || !status) return fail(ctx, BPMI_E_ARG, std::string(fn) + ": null argument");
  u32 k;
  if (!log2_exact(n, k) || k > IPAB_K_MAX) return fail(ctx, BPMI_E_ARG, std::string(fn) + ": n must be 2^k, k <= 22");
  IpaWireIn in;
  in.blobs = blobs; in.off = off; in.u = u; in.P = P; in.weights = weights; in.seed = seed;
  const IpawPlan pl = ipa_wire_plan(*ctx, k, protocol, n_proofs, in, true, d_hscale ? 1 : 0, ctx->ipap_t_budget);
  if (pl.err) return fail(ctx, pl.err, std::string(fn) + ": " + pl.msg);
  // the proofs' points are the decompression's and the preparation's to judge (status bit 1); the generators at level 2 by a
  // kernel whose verdict is read after the MSM's own synchronisation; a refused call leaves 0xFF.. in `out`
  PointCheck pc(ctx, fn, ctx->stream, ctx->opt_validate >= 1);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = ensure_stage_in(ctx, pl.total_bytes + 512);
  if (rc) return rc;
  char *base = (char *)ctx->stage_in;
  const IpabPlan &bp = pl.base;
  rc = ipaw_upload(ctx, pl, in);
  if (rc) return rc;
  IpaPackedIn statements;                          // what the expander cannot know: the statements and the weights
  statements.u = u; statements.P = P; statements.weights = weights;
  rc = ipap_upload_class(ctx, pl, statements, 0);
  if (rc) return rc;
  ipad::Params q;
  ipap_describe_class(ctx, pl, true, weights, seed, k, 2, n_proofs, (u32 *)(base + bp.o_rec), (u32 *)(base + bp.o_exsc), q);
  const IpawDev d = {pl, base, off[0]};
  ipaw_decompress_launch(ctx, d);
  rc = ipap_launch_kernels(ctx, q, pl.rows, pl.pairs, (u32 *)(base + bp.o_expt), (uint8_t *)base + pl.o_status,
                           [&](uint64_t first, u32 cnt) { ipaw_expand_launch(ctx, d, first, cnt); },
                           [&](uint64_t first, u32 cnt) {
                             hipLaunchKernelGGL(ipad::k_ipaw_verdicts, dim3((cnt + 255) / 256), dim3(256), 0, ctx->stream, q.roles, q.Pall, (const uint8_t *)d.badflag(),
                                                (const uint8_t *)d.ptflag(), (u64)first, cnt);
                           });
  if (rc) return rc;
  HIPCHK(ctx, hipMemcpyAsync(status, base + pl.o_status, n_proofs, hipMemcpyDeviceToHost, ctx->stream));
  rc = ipab_svector_launches(ctx, bp, d_hscale);
  if (rc) return rc;
  return ipa_verify_msm(ctx, pc, d_g, d_h, n, base + bp.o_sa, base + bp.o_sb, base + bp.o_expt, base + bp.o_exsc, bp.n_extra, false, true, out);
}

}  // extern "C"
