/* Fixed-base MSM through the C-ABI only (no Python, no torch, no HIP headers):
 *
 *   gcc -O2 -std=c99 -Iinclude examples/msm_fixed_c_abi.c -o msm_fixed_c_abi \
 *       python-bulletproofs_amd/libbpmi.so -Wl,-rpath,$PWD/python-bulletproofs_amd
 *   ./msm_fixed_c_abi 14 16 4        # log2 n, window bits, rows
 *
 * Builds n generators k_i * G on the GPU, hands them to bpmi_fixed_base_create_dev (which copies them and builds the table of their
 * multiples), and computes two MSMs over them with two different scalar vectors through the asynchronous pair
 * (bpmi_msm_fixed_dev_enqueue / bpmi_msm_finish), both in flight at once.  Every result is compared with bpmi_msm over the same
 * points and scalars and with the synchronous bpmi_msm_fixed_dev; the second vector is shorter than n (the missing scalars are 0). */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bpmi.h"

static uint64_t s = 88172645463325252ULL;
static uint64_t rnd(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }

static const uint8_t G_LE[64] = {
    0x98, 0x17, 0xF8, 0x16, 0x5B, 0x81, 0xF2, 0x59, 0xD9, 0x28, 0xCE, 0x2D, 0xDB, 0xFC, 0x9B, 0x02,
    0x07, 0x0B, 0x87, 0xCE, 0x95, 0x62, 0xA0, 0x55, 0xAC, 0xBB, 0xDC, 0xF9, 0x7E, 0x66, 0xBE, 0x79,
    0xB8, 0xD4, 0x10, 0xFB, 0x8F, 0xD0, 0x47, 0x9C, 0x19, 0x54, 0x85, 0xA6, 0x48, 0xB4, 0x17, 0xFD,
    0xA8, 0x08, 0x11, 0x0E, 0xFC, 0xFB, 0xA4, 0x5D, 0x65, 0xC4, 0xA3, 0x26, 0x77, 0xDA, 0x3A, 0x48};

#define CK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, bpmi_last_error(ctx)); return 1; } } while (0)

int main(int argc, char **argv) {
  const int logn = argc > 1 ? atoi(argv[1]) : 14;
  const uint32_t window_bits = argc > 2 ? (uint32_t)atoi(argv[2]) : 16, rows = argc > 3 ? (uint32_t)atoi(argv[3]) : 4;
  const uint64_t n = 1ull << logn, m = n - n / 3;              /* the second vector covers the first m generators only */
  bpmi_ctx *ctx = bpmi_ctx_create(0, NULL);
  if (!ctx) { fprintf(stderr, "no GPU: %s\n", bpmi_last_error(NULL)); return 2; }
  uint8_t *ks = malloc(32 * n), *es = malloc(64 * n), *gs = malloc(64 * n);
  for (uint64_t i = 0; i < n; i++) {
    for (int w = 0; w < 4; w++) { uint64_t a = rnd(), b = rnd(), c = rnd(); memcpy(ks + 32 * i + 8 * w, &a, 8); memcpy(es + 32 * i + 8 * w, &b, 8); memcpy(es + 32 * (n + i) + 8 * w, &c, 8); }
    ks[32 * i + 31] &= 0x3F;                                   /* < 2^254 < q; the scalars are any 256-bit values */
    memcpy(gs + 64 * i, G_LE, 64);
  }
  void *d_k, *d_g, *d_p, *d_e;
  CK(bpmi_malloc(ctx, 32 * n, &d_k)); CK(bpmi_malloc(ctx, 64 * n, &d_g)); CK(bpmi_malloc(ctx, 64 * n, &d_p)); CK(bpmi_malloc(ctx, 64 * n, &d_e));
  CK(bpmi_upload(ctx, d_k, ks, 32 * n)); CK(bpmi_upload(ctx, d_g, gs, 64 * n)); CK(bpmi_upload(ctx, d_e, es, 64 * n));
  CK(bpmi_ec_mul_batch_dev(ctx, d_g, d_k, n, d_p));            /* P_i = k_i G */
  CK(bpmi_download(ctx, gs, d_p, 64 * n));                     /* ... and on the host, for bpmi_msm */
  bpmi_fixed_base *fx = NULL;
  CK(bpmi_fixed_base_create_dev(ctx, d_p, n, window_bits, rows, &fx));
  CK(bpmi_free(ctx, d_p));                                     /* the object has its own copy */
  uint64_t info[8];
  CK(bpmi_fixed_base_info(fx, info));
  printf("n=%llu  c=%llu  W=%llu  rows=%llu  Wv=%llu  table %llu bytes  built in %.3f ms\n", (unsigned long long)info[0], (unsigned long long)info[1],
         (unsigned long long)info[2], (unsigned long long)info[3], (unsigned long long)info[4], (unsigned long long)info[5], 1e-3 * (double)info[6]);
  uint8_t want0[64], want1[64], got0[64], got1[64], sync0[64];
  CK(bpmi_msm(ctx, gs, es, n, want0));
  CK(bpmi_msm(ctx, gs, es + 32 * n, m, want1));
  CK(bpmi_msm_fixed_dev_enqueue(fx, 0, d_e, n));
  CK(bpmi_msm_fixed_dev_enqueue(fx, 1, (uint8_t *)d_e + 32 * n, m));
  CK(bpmi_msm_finish(ctx, 0, got0));
  CK(bpmi_msm_finish(ctx, 1, got1));
  CK(bpmi_msm_fixed_dev(fx, d_e, n, sync0));
  const int bad = memcmp(got0, want0, 64) != 0 || memcmp(got1, want1, 64) != 0 || memcmp(sync0, want0, 64) != 0 || memcmp(want0, want1, 64) == 0;
  printf("two fixed-base MSMs in flight against bpmi_msm: %s\n", bad ? "MISMATCH" : "ok");
  bpmi_fixed_base_destroy(fx);
  bpmi_free(ctx, d_k); bpmi_free(ctx, d_g); bpmi_free(ctx, d_e);
  bpmi_ctx_destroy(ctx);
  free(ks); free(es); free(gs);
  return bad;
}
