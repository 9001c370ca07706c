/* Inner-product arguments of TWO lengths over the prefixes of one generator list, proved by two batch provers and verified in ONE
 * call, through the C-ABI alone (no Python, no torch, no HIP headers):
 *
 *   gcc -O2 -std=c99 -Iinclude examples/ipa_prove_verify_mixed_c_abi.c -o ipa_prove_verify_mixed_c_abi \
 *       python-bulletproofs_amd/libbpmi.so -Wl,-rpath,$PWD/python-bulletproofs_amd
 *   ./ipa_prove_verify_mixed_c_abi [proofs_per_length [table_bits]]
 *
 * What it replaces: per length a loop of FastNIProver2(g[:n], h[:n], u, P, a, b, group).prove()
 * (src/innerproduct/inner_product_prover.py:48-110 of the reference) and a loop of Verifier2(g[:n], h[:n], u, P, proof).verify()
 * (src/innerproduct/inner_product_verifier.py:104-147).
 *   1. one list of 64 generators g, h and a u; bpmi_ipa_batch_prover_create over g[:8], h[:8] and over g[:64], h[:64];
 *   2. per prover: the statements P_p = <a_p, g> + <b_p, h> + <a_p, b_p> u and bpmi_ipa_prove_batch -- the packed arrays of one CLASS;
 *   3. bpmi_ipa_verify_batch_packed_mixed_dev over the two classes (given with the longer one LAST: any order of k is legal): both are
 *      prepared on the device in one launch, then one s-vector sum and ONE MSM over [g | h | extra].  The batch is valid iff every status
 *      byte is 0 and out is the identity;
 *   4. one transcript byte of one proof of the second class is flipped: the batch is rejected and the status byte at that proof's GLOBAL
 *      (class-major) index says which proof it was.
 * The generators here are multiples of the curve's base point (a demonstration, not a setup ceremony).
 * Exit code 0: the valid batch verified and the spoiled one was rejected at the right index; 1: a verdict was wrong; 2: error. */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bpmi.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static void small_scalar(uint8_t s[32], int bytes) { int i; memset(s, 0, 32); for (i = 0; i < bytes; i++) s[i] = (uint8_t)rnd(); }

/* the base point of secp256k1, x || y, little-endian coordinates */
static const uint8_t G_LE[64] = {
  0x98, 0x17, 0xF8, 0x16, 0x5B, 0x81, 0xF2, 0x59, 0xD9, 0x28, 0xCE, 0x2D, 0xDB, 0xFC, 0x9B, 0x02, 0x07, 0x0B, 0x87, 0xCE, 0x95, 0x62, 0xA0, 0x55,
  0xAC, 0xBB, 0xDC, 0xF9, 0x7E, 0x66, 0xBE, 0x79, 0xB8, 0xD4, 0x10, 0xFB, 0x8F, 0xD0, 0x47, 0x9C, 0x19, 0x54, 0x85, 0xA6, 0x48, 0xB4, 0x17, 0xFD,
  0xA8, 0x08, 0x11, 0x0E, 0xFC, 0xFB, 0xA4, 0x5D, 0x65, 0xC4, 0xA3, 0x26, 0x77, 0xDA, 0x3A, 0x48};

#define CK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, bpmi_last_error(ctx)); return 2; } } while (0)
#define NMAX 64u

/* one class: `count` proofs of n = 2^k elements over g[:n], h[:n], from a prover of its own */
static int prove_class(bpmi_ctx *ctx, uint32_t k, uint64_t count, const uint8_t *g, const uint8_t *h, const uint8_t *u, bpmi_ipa_packed_class *out) {
  const uint32_t n = 1u << k;
  const uint64_t ng = 2ull * n + 1;
  uint64_t i;
  bpmi_ipa_batch_prover *pv = NULL;
  CK(bpmi_ipa_batch_prover_create(ctx, n, g, h, u, NULL, &pv));
  uint8_t *pts = malloc(64 * ng), *sc = malloc(32 * ng);
  uint8_t *a = malloc(32ull * n * count), *b = malloc(32ull * n * count), *Pst = malloc(64 * count), *us = malloc(64 * count);
  memcpy(pts, g, 64ull * n); memcpy(pts + 64ull * n, h, 64ull * n); memcpy(pts + 128ull * n, u, 64);
  for (i = 0; i < (uint64_t)n * count; i++) { small_scalar(a + 32 * i, 31); small_scalar(b + 32 * i, 31); }
  for (i = 0; i < count; i++) {          /* P_p: one MSM over [g[:n] | h[:n] | u] */
    memcpy(sc, a + 32ull * n * i, 32ull * n);
    memcpy(sc + 32ull * n, b + 32ull * n * i, 32ull * n);
    CK(bpmi_sc_dot(ctx, a + 32ull * n * i, b + 32ull * n * i, n, sc + 64ull * n));
    CK(bpmi_msm(ctx, pts, sc, ng, Pst + 64 * i));
    memcpy(us + 64 * i, u, 64);
  }
  const uint64_t cap = count * bpmi_ipa_prove_batch_transcript_bytes(pv, 2, 0);
  uint8_t *ab = malloc(64 * count), *xs = malloc(32ull * k * count + 1), *LR = malloc(128ull * k * count + 1), *tr = malloc(cap + 1);
  uint64_t *soff = calloc(count + 1, 8), *tr_off = malloc(8 * (count + 1));
  CK(bpmi_ipa_prove_batch(pv, 2, count, a, b, NULL, NULL, NULL, soff, ab, xs, LR, NULL, tr, cap, tr_off));
  bpmi_ipa_batch_prover_destroy(pv);
  free(pts); free(sc); free(a); free(b); free(soff);
  memset(out, 0, sizeof(*out));
  out->k = k; out->n_proofs = count;
  out->ab = ab; out->xs = xs; out->LR = LR; out->transcripts = tr; out->tr_off = tr_off; out->start = NULL;
  out->u = us; out->P = Pst; out->c = NULL; out->head = NULL;
  return 0;
}

int main(int argc, char **argv) {
  const uint64_t count = argc > 1 ? strtoull(argv[1], NULL, 10) : 5;
  const int table_bits = argc > 2 ? atoi(argv[2]) : 0;
  uint64_t i, j;
  if (count < 2 || count > 30000) { fprintf(stderr, "2 .. 30000 proofs per length\n"); return 2; }
  bpmi_ctx *ctx = bpmi_ctx_create(0, NULL);
  if (!ctx) { fprintf(stderr, "bpmi_ctx_create: %s\n", bpmi_last_error(NULL)); return 2; }
  if (table_bits) CK(bpmi_set_option(ctx, "prover_table_bits", table_bits));
  /* the capacity: g, h (64 each) and u, 129 multiples of G */
  const uint64_t ng = 2ull * NMAX + 1;
  uint8_t *gpts = malloc(64 * ng), *gin = malloc(64 * ng), *gsc = malloc(32 * ng);
  for (i = 0; i < ng; i++) { memcpy(gin + 64 * i, G_LE, 64); small_scalar(gsc + 32 * i, 31); }
  CK(bpmi_ec_mul_batch(ctx, gin, gsc, ng, gpts));
  const uint8_t *g = gpts, *h = gpts + 64ull * NMAX, *u = gpts + 128ull * NMAX;
  /* class 0: n = 8, class 1: n = 64 */
  bpmi_ipa_packed_class cls[2];
  if (prove_class(ctx, 3, count, g, h, u, &cls[0])) return 2;
  if (prove_class(ctx, 6, count, g, h, u, &cls[1])) return 2;
  printf("%llu proofs of 8 and %llu proofs of 64 elements over the prefixes of one list of %u generators\n", (unsigned long long)count, (unsigned long long)count, NMAX);
  void *d_g = NULL, *d_h = NULL;
  CK(bpmi_malloc(ctx, 64ull * NMAX, &d_g));
  CK(bpmi_malloc(ctx, 64ull * NMAX, &d_h));
  CK(bpmi_upload(ctx, d_g, g, 64ull * NMAX));
  CK(bpmi_upload(ctx, d_h, h, 64ull * NMAX));
  const uint64_t total = 2 * count, spoiled = count + count / 2;          /* global index: class 1's proof count / 2 */
  uint8_t seed[32], out[64], zero[64] = {0}, *status = malloc(total);
  int verdicts[2], round, located = 0;
  for (round = 0; round < 2; round++) {
    for (j = 0; j < 32; j++) seed[j] = (uint8_t)rnd();   /* (a real verifier draws this from the system's CSPRNG) */
    if (round == 1) ((uint8_t *)cls[1].transcripts)[cls[1].tr_off[count / 2] + 8] ^= 1;      /* a byte of an L item */
    CK(bpmi_ipa_verify_batch_packed_mixed_dev(ctx, d_g, d_h, NULL, NMAX, 2, 2, cls, NULL, seed, out, status));
    uint64_t flagged = 0;
    for (i = 0; i < total; i++) flagged += status[i] != 0;
    verdicts[round] = !flagged && !memcmp(out, zero, 64);
    printf("mixed batch verification (%s): %s, %llu proofs flagged", round == 0 ? "as proved" : "one transcript byte changed", verdicts[round] ? "VALID" : "INVALID",
           (unsigned long long)flagged);
    if (round == 1) {
      located = flagged == 1 && status[spoiled] != 0;
      for (i = 0; i < total; i++) if (status[i]) printf(", proof %llu (class %d, its proof %llu)", (unsigned long long)i, i < count ? 0 : 1, (unsigned long long)(i % count));
    }
    printf("\n");
  }
  bpmi_free(ctx, d_g); bpmi_free(ctx, d_h);
  bpmi_ctx_destroy(ctx);
  return verdicts[0] && !verdicts[1] && located ? 0 : 1;
}
