/* Range proofs of TWO sizes proved in ONE call from ONE table and verified as ONE combination, through the C-ABI alone (no Python, no
 * torch, no HIP headers):
 *
 *   gcc -O2 -std=c99 -Iinclude examples/prove_verify_mixed_c_abi.c -o prove_verify_mixed_c_abi \
 *       python-bulletproofs_amd/libbpmi.so -Wl,-rpath,$PWD/python-bulletproofs_amd
 *   ./prove_verify_mixed_c_abi [proofs of 1 value [proofs of M values [bits [M [spoil]]]]]
 *
 * What a service that fills blocks of transactions does, and what it replaces: a loop of NIRangeProver(v, bits, g, h, gs[:bits],
 * hs[:bits], gamma, u, group, seed).prove() (/root/reference/src/rangeproofs/rangeproof_prover.py:35-91) and of
 * AggregNIRangeProver(vs, bits, g, h, gs, hs, gammas, u, group, seed).prove() (/root/reference/src/rangeproofs/rangeproof_aggreg_prover.py:36-146).
 *   1. bpmi_rp_prover_create_aggregated(bits, M): the tables of the LONGEST generator list, once -- the capacity;
 *   2. bpmi_rp_prove_batch_mixed: a class of single-value proofs over gs[:bits], hs[:bits] and a class of M-value proofs, one call;
 *   3. bpmi_rp_prover_commit_batch: every commitment V = v g + gamma h from the same tables;
 *   4. (the other side) bpmi_rp_batch_verify_mixed_dev over the two classes as they were written.
 * The generators are multiples of the curve's base point (a demonstration, not a setup ceremony).  spoil = 1 changes one commitment
 * after proving: the block must be rejected.  Exit code 0: proved and verified; 1: the block did not verify; 2: error. */
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

#define CK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #call, rc_, bpmi_last_error(ctx)); return 2; } } while (0)

int main(int argc, char **argv) {
  const uint64_t P1 = argc > 1 ? strtoull(argv[1], NULL, 10) : 48, PM = argc > 2 ? strtoull(argv[2], NULL, 10) : 5;
  const uint32_t bits = argc > 3 ? (uint32_t)atoi(argv[3]) : 16, M = argc > 4 ? (uint32_t)atoi(argv[4]) : 4;
  const int spoil = argc > 5 ? atoi(argv[5]) : 0;
  const uint32_t N = bits * M;                         /* the capacity's generators per side */
  const uint64_t count[2] = {P1, PM};
  const uint32_t m[2] = {1, M};
  uint32_t k[2] = {0, 0};
  uint64_t i;
  int c;
  if (!P1 || !PM || bits < 2) { fprintf(stderr, "both classes need a proof, and a value two bits\n"); return 2; }
  for (c = 0; c < 2; c++) while ((1u << k[c]) < bits * m[c]) k[c]++;
  bpmi_ctx *ctx = bpmi_ctx_create(0, NULL);
  if (!ctx) { fprintf(stderr, "bpmi_ctx_create: %s\n", bpmi_last_error(NULL)); return 2; }
  CK(bpmi_set_option(ctx, "prover_table_bits", 8));    /* (a demonstration: a small table) */
  /* generators: g, h, u, gs[0..N), hs[0..N) as multiples of G */
  const uint64_t ng = 3 + 2ull * N;
  uint8_t *gpts = malloc(64 * ng), *gin = malloc(64 * ng), *gsc = malloc(32 * ng);
  for (i = 0; i < ng; i++) { memcpy(gin + 64 * i, G_LE, 64); small_scalar(gsc + 32 * i, 31); }
  CK(bpmi_ec_mul_batch(ctx, gin, gsc, ng, gpts));
  const uint8_t *g = gpts, *h = gpts + 64, *u = gpts + 128, *gs = gpts + 192, *hs = gpts + 192 + 64 * (uint64_t)N;
  double t0 = now();
  bpmi_rp_prover *pv = NULL;
  CK(bpmi_rp_prover_create_aggregated(ctx, bits, M, g, h, u, gs, hs, &pv));
  printf("one prover for proofs of 1 .. %u values of %u bits: tables built in %.1f ms\n", M, bits, (now() - t0) * 1e3);
  /* inputs per class: values below 2^bits, blinding factors, seeds "class-<c>-proof-<i>" */
  bpmi_rp_prove_class cls[2];
  uint8_t *vals[2], *gams[2], *seeds[2];
  uint64_t *soff[2], cap = 0, total = P1 + PM;
  for (c = 0; c < 2; c++) {
    const uint64_t NV = count[c] * m[c];
    uint64_t spos = 0;
    vals[c] = calloc(NV, 32); gams[c] = malloc(32 * NV); seeds[c] = malloc(40 * count[c]); soff[c] = malloc(8 * (count[c] + 1));
    for (i = 0; i < NV; i++) {
      const uint64_t v = bits >= 64 ? rnd() : (rnd() & ((1ull << bits) - 1));
      memcpy(vals[c] + 32 * i, &v, 8);                 /* (little-endian host) */
      small_scalar(gams[c] + 32 * i, 31);
    }
    for (i = 0; i < count[c]; i++) {
      soff[c][i] = spos;
      spos += (uint64_t)sprintf((char *)seeds[c] + spos, "class-%d-proof-%llu", c, (unsigned long long)i);
    }
    soff[c][count[c]] = spos;
    cls[c].m = m[c]; cls[c].n_proofs = count[c]; cls[c].values = vals[c]; cls[c].gammas = gams[c]; cls[c].seeds = seeds[c]; cls[c].seed_off = soff[c];
    cap += count[c] * bpmi_rp_prove_batch_proof_bytes_class(pv, m[c], 0) + spos;
  }
  uint8_t *wire = NULL;
  uint64_t *ooff = malloc(8 * (total + 1));
  CK(bpmi_host_alloc(ctx, cap, (void **)&wire));       /* page-locked: the proofs land here straight from the device */
  CK(bpmi_rp_prove_batch_mixed(pv, 2, cls, wire, cap, ooff));      /* warm */
  t0 = now();
  CK(bpmi_rp_prove_batch_mixed(pv, 2, cls, wire, cap, ooff));
  const double dt = now() - t0;
  double ms[7];
  CK(bpmi_rp_prover_last_ms(pv, ms));
  printf("%llu + %llu proofs in one call: %.2f ms (device %.2f ms), %llu wire bytes\n", (unsigned long long)P1, (unsigned long long)PM, dt * 1e3, ms[6],
         (unsigned long long)ooff[total]);
  /* the commitments of both classes from the prover's tables, then the verifier's classes: the proofs are class-major in `wire` */
  uint8_t *V[2];
  bpmi_rp_class vc[2];
  uint64_t *boff[2], first = 0, pairs = 0;
  for (c = 0; c < 2; c++) {
    const uint64_t NV = count[c] * m[c], lo = ooff[first];
    V[c] = malloc(64 * NV);
    CK(bpmi_rp_prover_commit_batch(pv, NV, vals[c], gams[c], V[c]));
    boff[c] = malloc(8 * (count[c] + 1));
    for (i = 0; i <= count[c]; i++) boff[c][i] = ooff[first + i] - lo;
    vc[c].n_gens = bits * m[c]; vc[c].values_per_proof = m[c]; vc[c].n_proofs = count[c];
    vc[c].blobs = wire + lo; vc[c].blobs_len = ooff[first + count[c]] - lo; vc[c].blob_off = boff[c]; vc[c].v_points = V[c];
    pairs += count[c] * (m[c] + 6 + 2ull * k[c]);
    first += count[c];
  }
  if (spoil) memcpy(V[1] + 64 * (count[1] * M / 2), V[0], 64);
  void *d_gens = NULL, *d_pts = NULL, *d_sc = NULL;
  CK(bpmi_malloc(ctx, 64 * ng, &d_gens));
  CK(bpmi_malloc(ctx, 64 * pairs, &d_pts));
  CK(bpmi_malloc(ctx, 32 * pairs, &d_sc));
  CK(bpmi_upload(ctx, d_gens, gpts, 64 * ng));
  uint8_t seed[32], out[64], zero[64] = {0};
  for (i = 0; i < 32; i++) seed[i] = (uint8_t)rnd();   /* (a real verifier draws this from the system's CSPRNG) */
  int64_t bad = -1;
  t0 = now();
  CK(bpmi_rp_batch_verify_mixed_dev(ctx, 2, vc, N, NULL, seed, d_gens, d_pts, d_sc, out, &bad));
  const int valid = bad < 0 && !memcmp(out, zero, 64);
  printf("mixed batch verification: %s in %.2f ms\n", valid ? "VALID" : "INVALID", (now() - t0) * 1e3);
  bpmi_rp_prover_destroy(pv);
  bpmi_free(ctx, d_gens); bpmi_free(ctx, d_pts); bpmi_free(ctx, d_sc);
  bpmi_host_free(ctx, wire);
  bpmi_ctx_destroy(ctx);
  return valid ? 0 : 1;
}
