// msm_batch_plan_main.cpp -- the plan of a batched MSM (python-bulletproofs_amd/csrc/msm_batch_plan_host.hpp) printed as JSON, one line
// per shape: tests/test_msm_batch_plan_cpu.py compiles this with the host compiler and checks the lines.
//   msm_batch_plan_main <route> <vecs> <host_out> <nseg> <n0> <n1> <n2> <n_vec> [...]        (route, vecs: the two options)
#include <stdio.h>
#include <stdlib.h>

#include "msm_batch_plan_host.hpp"

int main(int argc, char **argv) {
  if (argc < 9 || (argc - 1) % 8) { fprintf(stderr, "usage: %s route vecs host_out nseg n0 n1 n2 n_vec ...\n", argv[0]); return 2; }
  for (int a = 1; a + 7 < argc; a += 8) {
    BpmiOptions opt;
    opt.opt_msm_batch_route = atoi(argv[a]);
    opt.opt_msm_batch_vecs = atoi(argv[a + 1]);
    const int host_out = atoi(argv[a + 2]);
    const u32 nseg = (u32)strtoul(argv[a + 3], nullptr, 10);
    const uint64_t n[3] = {strtoull(argv[a + 4], nullptr, 10), strtoull(argv[a + 5], nullptr, 10), strtoull(argv[a + 6], nullptr, 10)};
    const uint64_t n_vec = strtoull(argv[a + 7], nullptr, 10);
    const MsmBatchPlan p = msm_batch_plan(opt, nseg, n, n_vec, host_out != 0);
    printf("{\"err\": %d, \"msg\": ", p.err);
    if (p.msg) printf("\"%s\"", p.msg); else printf("null");           // (the plan's texts hold no quote or backslash)
    if (!p.err) {
      printf(", \"route\": %u, \"total\": %llu, \"n_vec\": %llu, \"threads\": %u, \"nmax\": %u, \"parts\": %u, \"W\": %u, \"vecs\": %u, \"launches\": %u", p.route,
             (unsigned long long)p.total, (unsigned long long)p.n_vec, p.threads, p.nmax, p.parts, p.W, p.vecs, p.launches);
      printf(", \"regions\": {\"E\": [%llu, %llu], \"out\": [%llu, %llu]}, \"total_bytes\": %llu", (unsigned long long)p.o_E, (unsigned long long)p.b_E,
             (unsigned long long)p.o_out, (unsigned long long)p.b_out, (unsigned long long)p.total_bytes);
      // every row range of up to 512 launches; of more, the first, the second and the last (one vector per launch would be 2^20 of them)
      printf(", \"ranges\": [");
      const bool all = p.launches <= 512;
      const u32 pick[3] = {0, 1, p.launches ? p.launches - 1 : 0};
      const u32 count = all ? p.launches : 3u;
      for (u32 i = 0; i < count; i++) {
        const u32 k = all ? i : pick[i];
        uint64_t v0 = 0;
        u32 cnt = 0;
        msmb_range(p, k, v0, cnt);
        printf("%s[%u, %llu, %u]", i ? ", " : "", k, (unsigned long long)v0, cnt);
      }
      printf("], \"min_vecs_by_parts\": [%u, %u, %u, %u], \"auto_parts_max\": %u, \"e_bytes_max\": %llu", msmb_min_vecs(1), msmb_min_vecs(2), msmb_min_vecs(3),
             msmb_min_vecs(4), MSMB_AUTO_PARTS_MAX, (unsigned long long)MSMB_E_BYTES_MAX);
    }
    printf("}\n");
  }
  return 0;
}
