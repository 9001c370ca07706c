/* Inner-product arguments of TWO lengths from ONE batch prover in ONE call, their statements from the same tables in one call, and
 * both classes verified in one call, through the C-ABI alone (no Python, no torch, no HIP headers):
 *
 *   gcc -O2 -std=c99 -Iinclude examples/ipa_prove_mixed_c_abi.c -o ipa_prove_mixed_c_abi \
 *       python-bulletproofs_amd/libbpmi.so -Wl,-rpath,$PWD/python-bulletproofs_amd
 *   ./ipa_prove_mixed_c_abi [proofs_per_length [table_bits]]
 *
 * What it replaces: per length a loop of FastNIProver2(g[:n], h[:n], u, P, a, b, group).prove()
 * (src/innerproduct/inner_product_prover.py:48-110 of the reference), of vector_commitment(g[:n], h[:n], a, b) + inner_product(a, b) * u
 * (src/utils/commitments.py:13) and of Verifier2(g[:n], h[:n], u, P, proof).verify() (src/innerproduct/inner_product_verifier.py:104-147)
 * -- and, on this library, one bpmi_ipa_batch_prover with a table of its own per length (examples/ipa_prove_verify_mixed_c_abi.c).
 *   1. one list of 64 generators g, h and a u; ONE bpmi_ipa_batch_prover_create over all 64: the capacity;
 *   2. bpmi_ipa_batch_prover_commit_batch_mixed: the statements P_p = <a_p, g[:n]> + <b_p, h[:n]> + <a_p, b_p> u of both classes;
 *   3. bpmi_ipa_prove_batch_mixed: the proofs of both classes, every protocol step one launch over both -- each class's outputs are the
 *      packed arrays of one class of the verifier;
 *   4. bpmi_ipa_verify_batch_packed_mixed_dev over the two classes: valid iff every status byte is 0 and out is the identity;
 *   5. one ab byte of one proof of the second class is flipped: the batch is rejected.
 * The generators here are multiples of the curve's base point (a demonstration, not a setup ceremony).
 * Exit code 0: the valid batch verified and the spoiled one was rejected; 1: a verdict was wrong; 2: error. */
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

int main(int argc, char **argv) {
  const uint64_t count = argc > 1 ? strtoull(argv[1], NULL, 10) : 5;
  const int table_bits = argc > 2 ? atoi(argv[2]) : 0;
  const uint32_t ks[2] = {3, 6};                 /* class 0: n = 8, class 1: n = 64 */
  uint64_t i, j;
  int c;
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
  bpmi_ipa_batch_prover *pv = NULL;
  CK(bpmi_ipa_batch_prover_create(ctx, NMAX, g, h, u, NULL, &pv));
  /* the classes: inputs, the statements' call, the proving call */
  bpmi_ipa_prove_class prove[2];
  bpmi_ipa_commit_class commit[2];
  bpmi_ipa_packed_class cls[2];
  memset(prove, 0, sizeof(prove)); memset(commit, 0, sizeof(commit)); memset(cls, 0, sizeof(cls));
  for (c = 0; c < 2; c++) {
    const uint32_t k = ks[c], n = 1u << k;
    uint8_t *a = malloc(32ull * n * count), *b = malloc(32ull * n * count), *Pst = malloc(64 * count), *us = malloc(64 * count);
    for (i = 0; i < (uint64_t)n * count; i++) { small_scalar(a + 32 * i, 31); small_scalar(b + 32 * i, 31); }
    for (i = 0; i < count; i++) memcpy(us + 64 * i, u, 64);
    const uint64_t cap = count * bpmi_ipa_prove_batch_transcript_bytes_class(pv, n, 2, 0);
    commit[c].n = n; commit[c].count = count; commit[c].a = a; commit[c].b = b; commit[c].t = NULL; commit[c].out = Pst;
    prove[c].n = n; prove[c].n_proofs = count; prove[c].a = a; prove[c].b = b;
    prove[c].seed_off = calloc(count + 1, 8);                  /* every transcript starts empty */
    prove[c].ab = malloc(64 * count); prove[c].xs = malloc(32ull * k * count); prove[c].LR = malloc(128ull * k * count);
    prove[c].transcripts = malloc(cap + 1); prove[c].cap = cap; prove[c].tr_off = malloc(8 * (count + 1));
    cls[c].k = k; cls[c].n_proofs = count;
    cls[c].ab = prove[c].ab; cls[c].xs = prove[c].xs; cls[c].LR = prove[c].LR; cls[c].transcripts = prove[c].transcripts; cls[c].tr_off = prove[c].tr_off;
    cls[c].u = us; cls[c].P = Pst;
  }
  CK(bpmi_ipa_batch_prover_commit_batch_mixed(pv, 1, 2, commit));
  CK(bpmi_ipa_prove_batch_mixed(pv, 2, 2, prove));
  double ms[4];
  CK(bpmi_ipa_batch_prover_last_ms(pv, ms));
  printf("%llu proofs of 8 and %llu proofs of 64 elements from one prover over %u generators in one call: %.3f ms on the device\n", (unsigned long long)count,
         (unsigned long long)count, NMAX, ms[3]);
  bpmi_ipa_batch_prover_destroy(pv);
  void *d_g = NULL, *d_h = NULL;
  CK(bpmi_malloc(ctx, 64ull * NMAX, &d_g));
  CK(bpmi_malloc(ctx, 64ull * NMAX, &d_h));
  CK(bpmi_upload(ctx, d_g, g, 64ull * NMAX));
  CK(bpmi_upload(ctx, d_h, h, 64ull * NMAX));
  const uint64_t total = 2 * count;
  uint8_t seed[32], out[64], zero[64] = {0}, *status = malloc(total);
  int verdicts[2], round;
  for (round = 0; round < 2; round++) {
    for (j = 0; j < 32; j++) seed[j] = (uint8_t)rnd();   /* (a real verifier draws this from the system's CSPRNG) */
    if (round == 1) prove[1].ab[64 * (count / 2)] ^= 1;   /* the low byte of a of class 1's proof count / 2 */
    CK(bpmi_ipa_verify_batch_packed_mixed_dev(ctx, d_g, d_h, NULL, NMAX, 2, 2, cls, NULL, seed, out, status));
    uint64_t flagged = 0;
    for (i = 0; i < total; i++) flagged += status[i] != 0;
    verdicts[round] = !flagged && !memcmp(out, zero, 64);
    printf("mixed batch verification (%s): %s\n", round == 0 ? "as proved" : "one scalar byte changed", verdicts[round] ? "VALID" : "INVALID");
  }
  bpmi_free(ctx, d_g); bpmi_free(ctx, d_h);
  bpmi_ctx_destroy(ctx);
  if (verdicts[0] && !verdicts[1]) printf("ok: one prover, one proving call, one statements call, one verifying call\n");
  return verdicts[0] && !verdicts[1] ? 0 : 1;
}
