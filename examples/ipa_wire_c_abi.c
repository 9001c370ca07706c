/* Inner-product arguments proved in one call, ENCODED in the wire format BPIP2 and verified FROM BYTES in one call, through the C-ABI
 * alone (no Python, no torch, no HIP headers):
 *
 *   gcc -O2 -std=c99 -Iinclude examples/ipa_wire_c_abi.c -o ipa_wire_c_abi \
 *       python-bulletproofs_amd/libbpmi.so -Wl,-rpath,$PWD/python-bulletproofs_amd
 *   ./ipa_wire_c_abi [n_proofs [n [table_bits]]]
 *
 * What it replaces: a loop of FastNIProver2(g, h, u, P, a, b, group).prove() (/root/reference/src/innerproduct/inner_product_prover.py:48-110),
 * a serialisation the reference does not have, and a loop of Verifier2(g, h, u, P, proof).verify()
 * (/root/reference/src/innerproduct/inner_product_verifier.py:104-147).
 *   1. bpmi_ipa_batch_prover_create, then the statements P_p = <a_p, g> + <b_p, h> + <a_p, b_p> u in one call
 *      (bpmi_ipa_batch_prover_commit_batch) and the proofs as packed arrays in one call (bpmi_ipa_prove_batch);
 *   2. bpmi_ipa_wire_encode: the packed arrays -> blobs of 78 + 98 k + 1 bytes each (the prefix of a proof from the empty transcript
 *      is "&") and their offsets -- what a prover would store or send;
 *   3. bpmi_ipa_verify_batch_wire_dev over the bytes: decompression and expansion in device memory, then the packed verifier's work.
 *      The batch is valid iff every status byte is 0 and out is the identity;
 *   4. one byte of one proof's `a` is flipped inside its blob: rejected through out (the bytes still parse); then one point's tag is
 *      set to 4: rejected through that proof's status byte (bit 1).
 * The generators here are multiples of the curve's base point (a demonstration, not a setup ceremony).
 * Exit code 0: the valid batch verified and both spoiled ones were rejected; 1: a verdict was wrong; 2: error. */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "bpmi.h"

static double now(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }
static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static void small_scalar(uint8_t s[32], int bytes) { int i; memset(s, 0, 32); for (i = 0; i < bytes; i++) s[i] = (uint8_t)rnd(); }

/* the base point of secp256k1, x || y, little-endian coordinates */
static const uint8_t G_LE[64] = {
  0x98, 0x17, 0xF8, 0x16, 0x5B, 0x81, 0xF2, 0x59, 0xD9, 0x28, 0xCE, 0x2D, 0xDB, 0xFC, 0x9B, 0x02, 0x07, 0x0B, 0x87, 0xCE, 0x95, 0x62, 0xA0, 0x55,
  0xAC, 0xBB, 0xDC, 0xF9, 0x7E, 0x66, 0xBE, 0x79, 0xB8, 0xD4, 0x10, 0xFB, 0x8F, 0xD0, 0x47, 0x9C, 0x19, 0x54, 0x85, 0xA6, 0x48, 0xB4, 0x17, 0xFD,
  0xA8, 0x08, 0x11, 0x0E, 0xFC, 0xFB, 0xA4, 0x5D, 0x65, 0xC4, 0xA3, 0x26, 0x77, 0xDA, 0x3A, 0x48};

#define CK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s -> %d: %s | %s\n", #call, rc_, bpmi_last_error(ctx), bpmi_last_error(NULL)); return 2; } } while (0)

int main(int argc, char **argv) {
  const uint64_t P = argc > 1 ? strtoull(argv[1], NULL, 10) : 1024;
  const uint32_t n = argc > 2 ? (uint32_t)atoi(argv[2]) : 64;
  const int table_bits = argc > 3 ? atoi(argv[3]) : 0;
  uint32_t k = 0;
  uint64_t i, j;
  while ((1u << k) < n) k++;
  if (P < 1 || (1u << k) != n) { fprintf(stderr, "n_proofs >= 1, n a power of two\n"); return 2; }
  bpmi_ctx *ctx = bpmi_ctx_create(0, NULL);
  if (!ctx) { fprintf(stderr, "bpmi_ctx_create: %s\n", bpmi_last_error(NULL)); return 2; }
  if (table_bits) CK(bpmi_set_option(ctx, "prover_table_bits", table_bits));
  /* generators g, h (n each) and u: 2n + 1 multiples of G */
  const uint64_t ng = 2ull * n + 1;
  uint8_t *gpts = malloc(64 * ng), *gin = malloc(64 * ng), *gsc = malloc(32 * ng);
  for (i = 0; i < ng; i++) { memcpy(gin + 64 * i, G_LE, 64); small_scalar(gsc + 32 * i, 31); }
  CK(bpmi_ec_mul_batch(ctx, gin, gsc, ng, gpts));
  const uint8_t *g = gpts, *h = gpts + 64ull * n, *u = gpts + 128ull * n;
  bpmi_ipa_batch_prover *pv = NULL;
  CK(bpmi_ipa_batch_prover_create(ctx, n, g, h, u, NULL, &pv));
  /* the witnesses, their statements and the proofs, packed (Protocol 2, every proof from the empty transcript) */
  uint8_t *a = malloc(32ull * n * P), *b = malloc(32ull * n * P), *Pst = malloc(64 * P), *us = malloc(64 * P);
  for (i = 0; i < (uint64_t)n * P; i++) { small_scalar(a + 32 * i, 31); small_scalar(b + 32 * i, 31); }
  for (i = 0; i < P; i++) memcpy(us + 64 * i, u, 64);
  CK(bpmi_ipa_batch_prover_commit_batch(pv, P, a, b, 1, NULL, Pst));
  const uint64_t cap = P * bpmi_ipa_prove_batch_transcript_bytes(pv, 2, 0);
  uint8_t *ab = malloc(64 * P), *xs = malloc(32ull * k * P + 1), *LR = malloc(128ull * k * P + 1), *tr = malloc(cap + 1);
  uint64_t *soff = calloc(P + 1, 8), *tr_off = malloc(8 * (P + 1));
  CK(bpmi_ipa_prove_batch(pv, 2, P, a, b, NULL, NULL, NULL, soff, ab, xs, LR, NULL, tr, cap, tr_off));
  const uint64_t packed_bytes = 64 * P + 32ull * k * P + 128ull * k * P + tr_off[P];
  /* the wire: one blob per proof, back to back */
  const uint64_t wire_cap = P * bpmi_ipa_wire_bytes(k, 0) + tr_off[P];
  uint8_t *blobs = malloc(wire_cap), *enc = malloc(P);
  uint64_t *off = malloc(8 * (P + 1));
  double t0 = now();
  CK(bpmi_ipa_wire_encode(k, 2, P, ab, k ? xs : NULL, k ? LR : NULL, tr, tr_off, NULL, blobs, wire_cap, off, enc));
  for (i = 0; i < P; i++) if (enc[i]) { fprintf(stderr, "proof %llu has no wire form\n", (unsigned long long)i); return 2; }
  printf("%llu proofs of %u elements encoded in %.2f ms: %llu bytes on the wire (%llu each), %llu packed\n", (unsigned long long)P, n, (now() - t0) * 1e3,
         (unsigned long long)off[P], (unsigned long long)bpmi_ipa_wire_bytes(k, 1), (unsigned long long)packed_bytes);
  if (off[P] != P * bpmi_ipa_wire_bytes(k, 1)) { fprintf(stderr, "unexpected blob length\n"); return 1; }
  /* the verifier's side: the generators in device memory once, then one call per batch of bytes */
  void *d_g = NULL, *d_h = NULL;
  CK(bpmi_malloc(ctx, 64ull * n, &d_g));
  CK(bpmi_malloc(ctx, 64ull * n, &d_h));
  CK(bpmi_upload(ctx, d_g, g, 64ull * n));
  CK(bpmi_upload(ctx, d_h, h, 64ull * n));
  uint8_t seed[32], out[64], zero[64] = {0}, *status = malloc(P);
  int verdicts[3], round;
  uint8_t *victim = blobs + off[P / 2];
  for (round = 0; round < 3; round++) {
    for (j = 0; j < 32; j++) seed[j] = (uint8_t)rnd();   /* (a real verifier draws this from the system's CSPRNG) */
    if (round == 1) victim[6 + 31] ^= 1;                 /* a wrong a (its last big-endian byte): every byte-level check still passes */
    if (round == 2) { victim[6 + 31] ^= 1; if (k) victim[6 + 32 * (2 + k)] = 4; }      /* the tag of L_0: no such encoding (k >= 1) */
    t0 = now();
    CK(bpmi_ipa_verify_batch_wire_dev(ctx, d_g, d_h, NULL, n, 2, P, blobs, off, us, Pst, NULL, seed, out, status));
    uint64_t flagged = 0;
    for (i = 0; i < P; i++) flagged += status[i] != 0;
    verdicts[round] = !flagged && !memcmp(out, zero, 64);
    printf("verification from bytes (%s): %s in %.2f ms, %llu proofs flagged\n", round == 0 ? "as encoded" : round == 1 ? "one a changed" : "one point tag changed",
           verdicts[round] ? "VALID" : "INVALID", (now() - t0) * 1e3, (unsigned long long)flagged);
    if (round == 2 && k && status[P / 2] != 2) { fprintf(stderr, "the spoiled proof's status is %d, not 2\n", status[P / 2]); return 1; }
  }
  bpmi_ipa_batch_prover_destroy(pv);
  bpmi_free(ctx, d_g); bpmi_free(ctx, d_h);
  bpmi_ctx_destroy(ctx);
  if (k == 0) return verdicts[0] && !verdicts[1] ? 0 : 1;             /* no round: no point to spoil */
  return verdicts[0] && !verdicts[1] && !verdicts[2] ? 0 : 1;
}
