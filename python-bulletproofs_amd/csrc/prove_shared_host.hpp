// prove_shared_host.hpp -- part of libbpmi (included by bpmi.hip; one translation unit).  HOST code.
// What the three batched provers share (rp_prove_host.hpp, rp_prove_mixed_host.hpp, ipa_prove_host.hpp): the device and page-locked
// buffers of a prover and their growth, the guard that keeps std::bad_alloc behind the C ABI, the scan of an input array for a scalar
// that is not reduced, and the launch of k_pv_msm in the instantiation of a lane width.
#pragma once

namespace rpp_host {

static inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// A prover's device arrays and its page-locked staging of the inputs / the results, kept between calls and grown on demand: a buffer
// that is too small is freed behind the stream's work and allocated anew with an eighth to spare
struct Buffers {
  void *buf = nullptr; size_t buf_bytes = 0;
  void *pin = nullptr; size_t pin_bytes = 0;
  int grow(bpmi_ctx *ctx, size_t dev_need, size_t pin_need) {
    if (dev_need > buf_bytes) {
      if (buf) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(buf)); buf = nullptr; buf_bytes = 0; }
      HIPCHK(ctx, hipMalloc(&buf, dev_need + dev_need / 8));
      buf_bytes = dev_need + dev_need / 8;
    }
    if (pin_need > pin_bytes) {
      if (pin) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipHostFree(pin)); pin = nullptr; pin_bytes = 0; }
      HIPCHK(ctx, hipHostMalloc(&pin, pin_need + pin_need / 8, hipHostMallocDefault));
      pin_bytes = pin_need + pin_need / 8;
    }
    return BPMI_OK;
  }
  void release() {                                 // (a prover's destroy: the stream is idle)
    if (buf) (void)hipFree(buf);
    if (pin) (void)hipHostFree(pin);
  }
};

// The C ABI never throws: a failed host allocation inside `body` -- a point list, the base lists, a plan, a std::string -- is
// BPMI_E_NOMEM under the entry point's name.  cleanup: what a create call undoes (the partial prover, *out)
template <class Body, class Cleanup>
static int guarded(bpmi_ctx *ctx, const char *fn, Body &&body, Cleanup &&cleanup) {
  try {
    return body();
  } catch (const std::bad_alloc &) {
    cleanup();
    return ctx ? fail(ctx, BPMI_E_NOMEM, std::string(fn) + ": out of host memory") : BPMI_E_NOMEM;
  }
}
template <class Body>
static int guarded(bpmi_ctx *ctx, const char *fn, Body &&body) { return guarded(ctx, fn, body, [] {}); }

// a 32-byte little-endian value below the group order?  (the kernels' mod-q arithmetic takes reduced operands: taux = ... + z^2 gamma)
static bool rp_scalar_reduced(const uint8_t le[32]) {
  static const uint8_t QLE[32] = {0x41, 0x41, 0x36, 0xD0, 0x8C, 0x5E, 0xD2, 0xBF, 0x3B, 0xA0, 0x48, 0xAF, 0xE6, 0xDC, 0xAE, 0xBA,
                                  0xFE, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF};
  for (int i = 31; i >= 0; i--) if (le[i] != QLE[i]) return le[i] < QLE[i];
  return false;
}
// The reference's provers take ModP values, reduced by construction (src/utils/utils.py:24-27); raw bytes are checked here.  Arrays of
// 32-byte scalars read side by side (p = nullptr: not given): the first scalar that is not below the group order -- the lowest index,
// at the same index the array named first -- as "name[i] is not below the group order", or empty
struct ScalarArray { const char *name; const uint8_t *p; uint64_t count; };
static std::string unreduced(std::initializer_list<ScalarArray> arrays) {
  const ScalarArray *who = nullptr;
  uint64_t at = ~0ull;
  for (const ScalarArray &A : arrays) {
    if (!A.p) continue;
    const uint64_t end = A.count < at ? A.count : at;
    uint64_t i = 0;
    while (i < end && rp_scalar_reduced(A.p + 32 * i)) i++;
    if (i < end) { who = &A; at = i; }
  }
  return who ? std::string(who->name) + "[" + std::to_string(at) + "] is not below the group order" : std::string();
}

// k_pv_msm over the jobs J, 2^gl lanes per job (gl: 1, 4 or 6)
static void launch_msm(hipStream_t st, const rpp::MsmJobs &J, const rpp::Tab &tab, int gl) {
  const dim3 grid((u32)((((uint64_t)J.njobs << gl) + 255) / 256));
  if (gl == 6) hipLaunchKernelGGL(rpp::k_pv_msm<6>, grid, dim3(256), 0, st, J, tab);
  else if (gl == 4) hipLaunchKernelGGL(rpp::k_pv_msm<4>, grid, dim3(256), 0, st, J, tab);
  else hipLaunchKernelGGL(rpp::k_pv_msm<1>, grid, dim3(256), 0, st, J, tab);
}

}  // namespace rpp_host
