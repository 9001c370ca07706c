// ipa_batch_plan_main.cpp -- the plan of a batch of inner-product verifications (python-bulletproofs_amd/csrc/ipa_batch_plan_host.hpp)
// printed as JSON, one line per shape: tests/test_ipa_batch_plan_cpu.py compiles this with the host compiler and checks the lines.
//   ipa_batch_plan_main <n> <n_proofs> <n_extra> <has_scale> [<n> <n_proofs> <n_extra> <has_scale> ...]
#include <stdio.h>
#include <stdlib.h>

#include "ipa_batch_plan_host.hpp"

int main(int argc, char **argv) {
  if (argc < 5 || (argc - 1) % 4) { fprintf(stderr, "usage: %s n n_proofs n_extra has_scale ...\n", argv[0]); return 2; }
  const BpmiOptions opt;
  for (int a = 1; a + 3 < argc; a += 4) {
    const unsigned long long n = strtoull(argv[a], nullptr, 10), np = strtoull(argv[a + 1], nullptr, 10), ne = strtoull(argv[a + 2], nullptr, 10);
    const int hs = atoi(argv[a + 3]);
    const IpabPlan p = ipa_batch_plan(opt, n, np, ne, hs);
    printf("{\"n\": %llu, \"n_proofs\": %llu, \"n_extra\": %llu, \"has_scale\": %d, \"err\": %d, \"msg\": ", n, np, ne, hs, p.err);
    if (p.msg) printf("\"%s\"", p.msg); else printf("null");           // (the plan's texts hold no quote or backslash)
    if (!p.err) {
      printf(", \"k\": %u, \"kl\": %u, \"kh\": %u, \"tab_entries\": %llu, \"rec_words\": %u, \"parts\": %u, \"per_part\": %u, \"direct\": %d", p.k, p.kl, p.kh,
             (unsigned long long)p.tab_entries, p.rec_words, p.parts, p.per_part, p.direct ? 1 : 0);
      const char *names[8] = {"sa", "sb", "rec", "tab", "part", "expt", "exsc", "scale"};
      const uint64_t offs[8] = {p.o_sa, p.o_sb, p.o_rec, p.o_tab, p.o_part, p.o_expt, p.o_exsc, p.o_scale};
      const uint64_t lens[8] = {p.b_sa, p.b_sb, p.b_rec, p.b_tab, p.b_part, p.b_expt, p.b_exsc, p.b_scale};
      printf(", \"regions\": {");
      for (int i = 0; i < 8; i++) printf("%s\"%s\": [%llu, %llu]", i ? ", " : "", names[i], (unsigned long long)offs[i], (unsigned long long)lens[i]);
      printf("}, \"total_bytes\": %llu, \"msm_pairs\": %llu, \"simds\": %u", (unsigned long long)p.total_bytes, (unsigned long long)p.msm_pairs, IPAB_SIMDS);
    }
    printf("}\n");
  }
  return 0;
}
