// h2c_host.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).
// Host side of the bulk hash to the curve (kernels: h2c_kernels.hpp; the C-ABI wrappers bpmi_ec_hash_* are in bpmi.hip): argument
// checks, staging, the launch shape, and the verdict.  Everything is ordered on the ctx stream, like bpmi_ec_decompress_batch[_dev].
#pragma once

#define H2C_MAX_MSG 65535u            // bytes per message (and per tail)
#define H2C_MAX_BYTES (1ull << 32)    // bytes per call
#define H2C_WAVES_FULL 3072u          // waves that fill the chip: 256 CUs x 4 SIMDs x 3 (the kernels' launch bounds)
#define H2C_PER_LANE_MAX 16u          // messages per lane of a span at most

// messages per wave of k_h2c_queue: whole rows of 64 (a 64-message call is ONE wave), as many rows as keep a large call at about
// H2C_WAVES_FULL waves (2^20 messages: 6 rows, 2 731 waves), 16 at most -- the idle tail of a span (about 7 iterations: the slowest
// of 64 messages) is paid once per span, against 2 iterations per row.  Measured at 2^21 messages: 8 rows 6.14 ms, 11 (this rule)
// 5.82, 16 5.71, 32 6.51.  One row is the plain loop's shape: h2c_run launches k_h2c_plain for it
static inline u32 h2c_span(uint64_t n, int opt_per_lane) {
  uint64_t rows = opt_per_lane > 0 ? (uint64_t)opt_per_lane : (n + 64ull * H2C_WAVES_FULL - 1) / (64ull * H2C_WAVES_FULL);
  if (rows < 1) rows = 1;
  if (!(opt_per_lane > 0) && rows > H2C_PER_LANE_MAX) rows = H2C_PER_LANE_MAX;
  return (u32)(64u * rows);
}

// The argument checks of both forms: nothing is read (but the offsets) or allocated before they pass.  *total = bytes to upload.
static int h2c_check(bpmi_ctx *ctx, bool range, const uint8_t *bytes, const uint64_t *msg_off, uint64_t tail_len, uint64_t lo, uint64_t hi, uint64_t n,
                     uint32_t max_tries, const void *out, uint64_t *total) {
  if (max_tries > 255u) return fail(ctx, BPMI_E_ARG, "max_tries must be 0 (= 255) or 1 .. 255");
  if (range) {
    if (lo > hi || hi > (1ull << 32)) return fail(ctx, BPMI_E_ARG, "range must satisfy lo <= hi <= 2^32");
    if (tail_len > H2C_MAX_MSG) return fail(ctx, BPMI_E_ARG, "tail longer than 65535 bytes");
    if (hi - lo > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
    if ((tail_len && !bytes) || (hi > lo && !out)) return fail(ctx, BPMI_E_ARG, "null argument");
    *total = tail_len;
    return BPMI_OK;
  }
  if (n > BPMI_MAX_N) return fail(ctx, BPMI_E_ARG, "n exceeds BPMI_MAX_N");
  if (n == 0) { *total = 0; return BPMI_OK; }
  if (!msg_off || !out) return fail(ctx, BPMI_E_ARG, "null argument");
  for (uint64_t i = 0; i < n; i++) {
    if (msg_off[i + 1] < msg_off[i]) return fail(ctx, BPMI_E_ARG, "message offsets decrease at index " + std::to_string(i));
    if (msg_off[i + 1] - msg_off[i] > H2C_MAX_MSG) return fail(ctx, BPMI_E_ARG, "message " + std::to_string(i) + " is longer than 65535 bytes");
  }
  if (msg_off[n] > H2C_MAX_BYTES) return fail(ctx, BPMI_E_ARG, "more than 4 GiB of messages");
  if (msg_off[n] && !bytes) return fail(ctx, BPMI_E_ARG, "null argument");
  *total = msg_off[n];
  return BPMI_OK;
}

// n messages -> n points in d_out (device memory) or, with d_out null, in out (host memory); tries: host memory or null
static int h2c_run(bpmi_ctx *ctx, bool range, const uint8_t *bytes, uint64_t total, const uint64_t *msg_off, uint64_t lo, uint64_t n, uint32_t max_tries,
                   void *d_out, uint8_t *out, uint8_t *tries) {
  if (n == 0) return BPMI_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // staging: the bytes | the offsets (batch form) | first_bad | tries | the points (host output)
  const size_t o_off = align_up(total, 256), o_bad = o_off + (range ? 0 : align_up(8 * (n + 1), 256)), o_tries = o_bad + 256, o_pts = o_tries + align_up(n, 256);
  int rc = ensure_stage_in(ctx, o_pts + (d_out ? 0 : 64 * n));
  if (rc) return rc;
  char *base = (char *)ctx->stage_in;
  if (total) HIPCHK(ctx, h2d(ctx, base, bytes, total, ctx->stream));         // (batch form: bytes[0, msg_off[n]), the offsets index it as they are)
  if (!range) HIPCHK(ctx, h2d(ctx, base + o_off, msg_off, 8 * (n + 1), ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(base + o_bad, 0xFF, 4, ctx->stream));
  H2cArgs a;
  a.bytes = (const uint8_t *)base;
  a.off = (const u64 *)(base + o_off);
  a.lo = lo;
  a.tail_len = (u32)total;
  a.n = (u32)n;
  a.max_tries = max_tries ? max_tries : 255u;
  a.span = h2c_span(n, ctx->opt_h2c_per_lane);
  a.out = (u32 *)(d_out ? d_out : base + o_pts);
  a.tries = (uint8_t *)(base + o_tries);
  a.first_bad = (u32 *)(base + o_bad);
  // One message per lane is all a call of up to 64 x H2C_WAVES_FULL messages needs to put a wave on every SIMD, and there the call lasts
  // as long as its slowest message (17 candidates among 2^16), which no schedule shortens: the plain loop is the kernel for that shape
  // (2^16: 1.66 ms against 1.88 for the queue at one message per lane, profiles/r09_hash_to_curve.txt).  The queue takes over where
  // lanes get several messages each (2^21: 5.8 ms against 13.4).
  const bool plain = ctx->opt_h2c_plain || (ctx->opt_h2c_per_lane == 0 && a.span == 64u);
  {
    StageTimer t(ctx, ST_MISC);
    if (plain) {
      const dim3 grid((u32)((n + 255) / 256));
      if (range) hipLaunchKernelGGL(k_h2c_plain<true>, grid, dim3(256), 0, ctx->stream, a);
      else hipLaunchKernelGGL(k_h2c_plain<false>, grid, dim3(256), 0, ctx->stream, a);
    } else {
      const uint64_t waves = (n + a.span - 1) / a.span;
      const dim3 grid((u32)((waves + 3) / 4));
      if (range) hipLaunchKernelGGL(k_h2c_queue<true>, grid, dim3(256), 0, ctx->stream, a);
      else hipLaunchKernelGGL(k_h2c_queue<false>, grid, dim3(256), 0, ctx->stream, a);
    }
  }
  HIPCHK(ctx, hipGetLastError());
  u32 first_bad = ~0u;
  HIPCHK(ctx, hipMemcpyAsync(&first_bad, base + o_bad, 4, hipMemcpyDeviceToHost, ctx->stream));
  if (tries) HIPCHK(ctx, hipMemcpyAsync(tries, base + o_tries, n, hipMemcpyDeviceToHost, ctx->stream));
  if (!d_out) HIPCHK(ctx, hipMemcpyAsync(out, base + o_pts, 64 * n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  // an identity must never pass silently for a generator: without a tries array the first message without a point fails the call
  if (!tries && first_bad != ~0u)
    return fail(ctx, BPMI_E_STATE, "message " + std::to_string(first_bad) + " has no point within " + std::to_string(a.max_tries) + " candidates");
  return BPMI_OK;
}
