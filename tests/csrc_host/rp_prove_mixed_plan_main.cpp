// rp_prove_mixed_plan_main.cpp -- the plan of a mixed call of the batched range-proof prover
// (python-bulletproofs_amd/csrc/rp_prove_mixed_plan_host.hpp) printed as JSON: tests/test_rp_prove_mixed_plan_cpu.py compiles this with
// the host compiler under the sanitizers and checks the lines.
//   rp_prove_mixed_plan_main bases <n> <N> [<n> <N> ...]                      one line per pair: rpp_class_bases(n, N)
//   rp_prove_mixed_plan_main plan <bits> <M> <wire format> <job lanes> [<m>:<count>:<seed total>:<seed max> ...]     one line: the plan
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rp_prove_mixed_plan_host.hpp"

#define U(x) ((unsigned long long)(x))

int main(int argc, char **argv) {
  if (argc >= 2 && !strcmp(argv[1], "bases") && argc % 2 == 0) {
    for (int a = 2; a + 1 < argc; a += 2) {
      const u32 n = (u32)strtoul(argv[a], nullptr, 10), N = (u32)strtoul(argv[a + 1], nullptr, 10);
      const std::vector<unsigned short> bl = rpp_class_bases(n, N);
      printf("{\"n\": %u, \"N\": %u, \"len\": %llu, \"bases\": [", n, N, U(rpp_class_bases_len(n)));
      for (size_t i = 0; i < bl.size(); i++) printf(i ? ",%u" : "%u", (unsigned)bl[i]);
      printf("]}\n");
    }
    return 0;
  }
  if (argc < 6 || strcmp(argv[1], "plan")) { fprintf(stderr, "usage: %s bases n N ... | plan bits M format lanes m:count:seed_total:seed_max ...\n", argv[0]); return 2; }
  const u32 nbits = (u32)strtoul(argv[2], nullptr, 10), M = (u32)strtoul(argv[3], nullptr, 10);
  const int fmt = atoi(argv[4]), lanes = atoi(argv[5]);
  std::vector<RppmClassIn> in;
  for (int a = 6; a < argc; a++) {
    RppmClassIn k;
    unsigned long long m = 0, count = 0, st = 0, sm = 0;
    if (sscanf(argv[a], "%llu:%llu:%llu:%llu", &m, &count, &st, &sm) != 4) { fprintf(stderr, "bad class %s\n", argv[a]); return 2; }
    k.m = (u32)m; k.count = count; k.seed_total = st; k.seed_max = sm;
    in.push_back(k);
  }
  const RppmPlan p = rpp_mixed_plan(nbits, M, 12, (u32)in.size(), in.data(), fmt, lanes);
  printf("{\"err\": %d, \"msg\": \"%s\"", p.err, p.msg.c_str());             // (the plan's texts hold no quote or backslash)
  if (!p.err) {
    printf(", \"N\": %u, \"k_max\": %u, \"nsteps\": %u, \"n_proofs\": %llu, \"total_out\": %llu, \"seed_bytes\": %llu", p.N, p.k_max, p.nsteps, U(p.n_proofs), U(p.total_out), U(p.seed_bytes));
    printf(", \"in_bytes\": %llu, \"need\": %llu, \"batch_slot\": %u, \"jobs_slot\": %u, \"unit_bytes\": %llu", U(p.in_bytes), U(p.need), RPPM_BATCH_SLOT, RPPM_JOBS_SLOT, U(sizeof(RppmUnit)));
    printf(", \"call_regions\": {\"seeds\": [%llu, %llu], \"soff\": [%llu, %llu], \"ooff\": [%llu, %llu], \"batch\": [%llu, %llu], \"jobs\": [%llu, %llu], \"units\": [%llu, %llu], \"out\": [%llu, %llu]}",
           U(p.o_seeds), U(p.seed_bytes + 16), U(p.o_soff), U(8 * (p.n_proofs + 1)), U(p.o_ooff), U(8 * (p.n_proofs + 1)), U(p.o_batch), U((size_t)RPPM_BATCH_SLOT * p.cls.size()),
           U(p.o_jobs), U((size_t)RPPM_JOBS_SLOT * p.jobs.size()), U(p.o_units), U(sizeof(RppmUnit) * p.units.size()), U(p.o_out), U(p.total_out + 16));
    printf(", \"classes\": [");
    for (size_t c = 0; c < p.cls.size(); c++) {
      const RppmClass &q = p.cls[c];
      const unsigned long long P = q.count, n = q.n, k = q.k;
      printf("%s{\"m\": %u, \"n\": %u, \"k\": %u, \"NT\": %u, \"per_block\": %u, \"npt\": %u, \"count\": %llu, \"first\": %llu, \"dig0_stride\": %u, \"tr_stride\": %u", c ? ", " : "", q.m, q.n,
             q.k, q.NT, q.per_block, q.npt, P, U(q.first), q.dig0_stride, q.tr_stride);
      printf(", \"bases_off\": %llu, \"seed_at\": %llu, \"out_at\": %llu, \"out_bytes\": %llu, \"fixed_bytes\": %llu, \"input\": [\"dig0\", \"dlen\", \"val\", \"gam\"], \"regions\": {", U(q.bases_off),
             U(q.seed_at), U(q.out_at), U(q.out_bytes), U(q.fixed_bytes));
      // every array of rpp::Batch: [offset, bytes]
      printf("\"dig0\": [%llu, %llu], \"dlen\": [%llu, %llu], \"val\": [%llu, %llu], \"gam\": [%llu, %llu]", U(q.o_dig0), P * q.dig0_stride, U(q.o_dlen), 4 * P, U(q.o_val), 32 * P * q.m, U(q.o_gam),
             32 * P * q.m);
      printf(", \"tr\": [%llu, %llu], \"trlen\": [%llu, %llu], \"slr\": [%llu, %llu], \"alpha\": [%llu, %llu], \"chal\": [%llu, %llu], \"tau\": [%llu, %llu], \"tsc\": [%llu, %llu]", U(q.o_tr),
             P * q.tr_stride, U(q.o_trlen), 4 * P, U(q.o_slr), 32 * P * (2 * n + 1), U(q.o_alpha), 32 * P, U(q.o_chal), 128 * P, U(q.o_tau), 64 * P, U(q.o_tsc), 128 * P);
      printf(", \"res\": [%llu, %llu], \"xs\": [%llu, %llu], \"xr\": [%llu, %llu], \"a\": [%llu, %llu], \"b\": [%llu, %llu], \"cg\": [%llu, %llu], \"hf\": [%llu, %llu]", U(q.o_res), 160 * P,
             U(q.o_xs), 32 * P * k, U(q.o_xr), 64 * P, U(q.o_a), 32 * P * n, U(q.o_b), 32 * P * n, U(q.o_cg), 32 * P * n, U(q.o_hf), 32 * P * n);
      printf(", \"jsc\": [%llu, %llu], \"jout\": [%llu, %llu], \"pts\": [%llu, %llu]}}", U(q.o_jsc), 32 * P * (2 * n + 2), U(q.o_jout), 288 * P, U(q.o_pts), 64 * P * q.npt);
    }
    printf("], \"launches\": [");
    for (size_t i = 0; i < p.launches.size(); i++) {
      const RppmLaunch &L = p.launches[i];
      printf("%s{\"name\": \"%s\", \"step\": %u, \"threads\": %u, \"gl\": %u, \"per\": %u, \"slot0\": %u, \"slot_step\": %u, \"step_k\": %u, \"round\": %u, \"first\": %u, \"blocks\": %u, \"units\": [",
             i ? ", " : "", rppm_kind_name(L.kind), L.step, L.threads, L.gl, L.per, L.slot0, L.slot_step, L.step_k, L.round, L.first, L.blocks);
      for (u32 u = 0; u < L.n_units; u++) printf("%s[%u, %u]", u ? ", " : "", p.units[L.first_unit + u].cls, p.units[L.first_unit + u].first);
      printf("]}");
    }
    printf("], \"jobs\": [");
    for (size_t i = 0; i < p.jobs.size(); i++) {
      const RppmJobs &j = p.jobs[i];
      printf("%s[%u, %u, %u, %u, %u, %u, %u]", i ? ", " : "", j.njobs, j.ntypes, j.T, j.stride, j.base_off, j.from_slr, j.from_tsc);
    }
    printf("]");
  }
  printf("}\n");
  return 0;
}
