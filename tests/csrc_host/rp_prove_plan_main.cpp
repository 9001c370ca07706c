// rp_prove_plan_main.cpp -- the batched prover's plan (python-bulletproofs_amd/csrc/rp_prove_plan_host.hpp) printed as JSON, one line per
// shape: tests/test_rp_prove_plan_cpu.py compiles this with the host compiler and checks the lines.
//   rp_prove_plan_main <bits> <values> <prover_table_bits> [<bits> <values> <prover_table_bits> ...]
//   rp_prove_plan_main layout <bits> <values> <proofs> <seed total> <seed max> [...]      one line per shape: rpp_layout (wire format 2)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rp_prove_plan_host.hpp"

static void print_text(const char *s) {
  if (!s) { printf("null"); return; }
  printf("\"%s\"", s);                       // (the plan's texts hold no quote or backslash)
}

// every array of rpp::Batch as "name": [offset, bytes]; the byte sizes are stated here, apart from the plan's
static void print_regions(const RppRegions &at, const RppGeom &g, const RppStrides &s, unsigned long long P) {
  const unsigned long long n = g.n, k = g.k;
#define U(x) ((unsigned long long)(x))
  printf("\"dig0\": [%llu, %llu], \"dlen\": [%llu, %llu], \"val\": [%llu, %llu], \"gam\": [%llu, %llu]", U(at.o_dig0), P * s.dig0_stride, U(at.o_dlen), 4 * P, U(at.o_val), 32 * P * g.m, U(at.o_gam),
         32 * P * g.m);
  printf(", \"tr\": [%llu, %llu], \"trlen\": [%llu, %llu], \"slr\": [%llu, %llu], \"alpha\": [%llu, %llu], \"chal\": [%llu, %llu], \"tau\": [%llu, %llu], \"tsc\": [%llu, %llu]", U(at.o_tr),
         P * s.tr_stride, U(at.o_trlen), 4 * P, U(at.o_slr), 32 * P * (2 * n + 1), U(at.o_alpha), 32 * P, U(at.o_chal), 128 * P, U(at.o_tau), 64 * P, U(at.o_tsc), 128 * P);
  printf(", \"res\": [%llu, %llu], \"xs\": [%llu, %llu], \"xr\": [%llu, %llu], \"a\": [%llu, %llu], \"b\": [%llu, %llu], \"cg\": [%llu, %llu], \"hf\": [%llu, %llu]", U(at.o_res), 160 * P,
         U(at.o_xs), 32 * P * k, U(at.o_xr), 64 * P, U(at.o_a), 32 * P * n, U(at.o_b), 32 * P * n, U(at.o_cg), 32 * P * n, U(at.o_hf), 32 * P * n);
  printf(", \"jsc\": [%llu, %llu], \"jout\": [%llu, %llu], \"pts\": [%llu, %llu]", U(at.o_jsc), 32 * P * (2 * n + 2), U(at.o_jout), 288 * P, U(at.o_pts), 64 * P * g.npt);
#undef U
}

int main(int argc, char **argv) {
  if (argc >= 2 && !strcmp(argv[1], "layout") && argc > 2 && (argc - 2) % 5 == 0) {
    for (int a = 2; a + 4 < argc; a += 5) {
      const uint32_t nbits = (uint32_t)strtoul(argv[a], nullptr, 10), m = (uint32_t)strtoul(argv[a + 1], nullptr, 10);
      const unsigned long long P = strtoull(argv[a + 2], nullptr, 10), st = strtoull(argv[a + 3], nullptr, 10), sm = strtoull(argv[a + 4], nullptr, 10);
      const RppGeom g = rpp_geom(nbits, m);
      const unsigned long long total_out = P * rpp_fixed_bytes(g.k, 2) + st;
      const RppLayout L = rpp_layout(g, (size_t)P, (size_t)st, sm, total_out, 81);
      printf("{\"bits\": %u, \"values\": %u, \"count\": %llu, \"seed_total\": %llu, \"seed_max\": %llu, \"total_out\": %llu, \"dig0_stride\": %u, \"tr_stride\": %u, \"in_bytes\": %llu, \"need\": %llu", nbits, m,
             P, st, sm, total_out, L.dig0_stride, L.tr_stride, (unsigned long long)L.in_bytes, (unsigned long long)L.need);
      printf(", \"call_regions\": {\"seeds\": [%llu, %llu], \"soff\": [%llu, %llu], \"ooff\": [%llu, %llu], \"out\": [%llu, %llu]}, \"regions\": {", (unsigned long long)L.o_seeds, st + 16,
             (unsigned long long)L.o_soff, 8 * (P + 1), (unsigned long long)L.o_ooff, 8 * (P + 1), (unsigned long long)L.o_out, total_out + 16);
      print_regions(L, g, L, P);
      printf("}}\n");
    }
    return 0;
  }
  if (argc < 4 || (argc - 1) % 3) { fprintf(stderr, "usage: %s bits values table_bits ...\n", argv[0]); return 2; }
  for (int a = 1; a + 2 < argc; a += 3) {
    const uint32_t nbits = (uint32_t)strtoul(argv[a], nullptr, 10), m = (uint32_t)strtoul(argv[a + 1], nullptr, 10);
    const int tw = atoi(argv[a + 2]);
    const RppPlan p = rpp_plan(nbits, m, tw);
    printf("{\"bits\": %u, \"values\": %u, \"opt_tw\": %d, \"err\": %d, \"msg\": ", nbits, m, tw, p.err);
    print_text(p.msg);
    if (!p.err) {
      printf(", \"n\": %u, \"k\": %u, \"NT\": %u, \"per_block\": %u, \"nbases\": %u, \"tw\": %u, \"wt\": %u, \"bt\": %u, \"table_bytes\": %llu, \"max_proofs\": %llu",
             p.n, p.k, p.NT, p.per_block, p.nbases, p.tw, p.wt, p.bt, (unsigned long long)p.table_bytes, (unsigned long long)p.max_proofs);
      printf(", \"off_S\": %u, \"off_T\": %u, \"off_P\": %u, \"off_round\": %u, \"bases\": [", p.off_S, p.off_T, p.off_P, p.off_round);
      for (size_t i = 0; i < p.bases.size(); i++) printf(i ? ",%u" : "%u", (unsigned)p.bases[i]);
      printf("], \"batch_errors\": {");
      const unsigned long long counts[] = {1, p.max_proofs, p.max_proofs + 1, PROVER_PROOFS_MAX, PROVER_PROOFS_MAX + 1};
      for (int i = 0; i < 5; i++) { printf(i ? ", \"%llu\": " : "\"%llu\": ", counts[i]); print_text(rpp_batch_error(p.max_proofs, counts[i])); }
      printf("}, \"job_lanes\": [");
      const unsigned long long jobs[] = {1, 16, PROVER_WAVE_JOBS_MAX, PROVER_WAVE_JOBS_MAX + 1, 1ull << 21};
      const int opts[] = {0, 16, 64};
      for (int i = 0; i < 5; i++) for (int o = 0; o < 3; o++) printf(i || o ? ", [%llu, %d, %d]" : "[%llu, %d, %d]", jobs[i], opts[o], 1 << rpp_job_lanes_log2(p.n, jobs[i], opts[o]));
      printf("], \"wave_jobs_max\": %u", PROVER_WAVE_JOBS_MAX);
    }
    printf("}\n");
  }
  return 0;
}
