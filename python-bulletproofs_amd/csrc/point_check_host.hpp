// point_check_host.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).
// The on-curve check of caller-supplied points (option "validate_points"), once: every entry point that checks holds one PointCheck.
//
// The reference can never hand an off-curve point to multiexp: fastecdsa's Point constructor rejects it (reached from
// /root/reference/src/utils/utils.py:119-131), and ec.py keeps that check for Python callers.  A C caller hands in raw bytes, so
// the entry points that take HOST pointers check them here (level 1, the default; level 2: the synchronous _dev entry points as
// well; 0: never): the identity (64 zero bytes) or x, y < p with y^2 = x^3 + 7.  Large arrays: k_ec_validate queued behind the
// upload, its verdict (the smallest bad index) copied to a page-locked word that is read after the call's own synchronisation --
// no extra wait; the call then fails with BPMI_E_ARG and writes NO result.  A few points: checked on the host.
// What a refused call leaves in its output is the entry point's business: a PointCheck never writes a caller's buffer.
#pragma once

#define VALIDATE_HOST_MAX 64u          // up to this many points an entry point with a host copy of them checks on the host
#define POINT_CHECK_ARRAYS 4u          // arrays one call may queue; array t's verdict is (t << 28) | index of its first bad point
static_assert(BPMI_MAX_N <= (1ull << 28), "an index into the largest array must fit below the verdict word's tag");
static_assert(POINT_CHECK_ARRAYS <= 15u, "every tagged verdict must stay below the 'no bad point' word 0xFFFFFFFF");

// One call's check.  An object that is off does nothing and returns BPMI_OK everywhere.  Order of use: host() at any time;
// queue() for every device array, fetch() once behind them, and verdict() after the CALLER has synchronised `st`.
struct PointCheck {
  bpmi_ctx *ctx; const char *fn; hipStream_t st; bool on;
  const char *names[POINT_CHECK_ARRAYS];          // names[t]: what the array queued t-th is called in the message
  u32 queued = 0;
  int setup = BPMI_OK;                            // the first failure of queue(), reported by fetch()
  PointCheck(bpmi_ctx *c, const char *fn_, hipStream_t st_, bool on_) : ctx(c), fn(fn_), st(st_), on(on_) {}

  int refuse(const char *name, uint64_t i) const {
    return fail(ctx, BPMI_E_ARG, std::string(fn) + ": " + name + "[" + std::to_string(i) + "] is not a point of the curve");
  }
  // pts[0 .. n) in host memory, now
  int host(const uint8_t *pts, uint64_t n, const char *name) const {
    for (uint64_t i = 0; on && i < n; i++) {
      u32 w[16];
      memcpy(w, pts + 64 * i, 64);
      if (!wire_point_valid(w)) return refuse(name, i);
    }
    return BPMI_OK;
  }
  // the verdict words (allocated at a ctx's first check), reset on the stream before the call's first check kernel
  int begin() {
    if (!ctx->vflag) {
      HIPCHK(ctx, hipHostMalloc((void **)&ctx->vflag, 64, hipHostMallocDefault));
      HIPCHK(ctx, hipMalloc((void **)&ctx->vflag_dev, 256));
    }
    *ctx->vflag = 0xFFFFFFFFu;
    HIPCHK(ctx, hipMemsetAsync(ctx->vflag_dev, 0xFF, 4, st));
    return BPMI_OK;
  }
  // d_pts[0 .. n) on the device, behind what is already queued on the stream; arrays are tagged in queue order
  void queue(const void *d_pts, uint64_t n, const char *name) {
    if (!on || !n || setup) return;
    if (queued == POINT_CHECK_ARRAYS) { setup = fail(ctx, BPMI_E_STATE, std::string(fn) + ": too many point arrays in one check"); return; }
    if (!queued && (setup = begin())) return;
    names[queued] = name;
    hipLaunchKernelGGL(k_ec_validate, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, (const u32 *)d_pts, (u32)n, queued << 28, ctx->vflag_dev);
    queued++;
  }
  // the copy of the verdict word, behind the check kernels
  int fetch() {
    if (setup || !queued) return setup;
    HIPCHK(ctx, hipMemcpyAsync(ctx->vflag, ctx->vflag_dev, 4, hipMemcpyDeviceToHost, st));
    return BPMI_OK;
  }
  // after the stream has been synchronised.  Nothing queued: the word may hold an earlier call's verdict and is not read
  int verdict() const {
    if (!queued) return BPMI_OK;
    const u32 v = *ctx->vflag;
    if (v == 0xFFFFFFFFu) return BPMI_OK;
    return refuse(names[v >> 28], v & 0x0FFFFFFFu);
  }
};
