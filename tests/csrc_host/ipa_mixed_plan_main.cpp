// ipa_mixed_plan_main.cpp -- the plan of a batch of inner-product verifications of different lengths
// (python-bulletproofs_amd/csrc/ipa_mixed_plan_host.hpp) printed as JSON, one line per case: tests/test_ipa_mixed_plan_cpu.py compiles this
// with the host compiler and checks the lines.  For a case of one length the line also carries per_part / parts of ipa_batch_plan.
// Input (standard input, whitespace separated):
//   <cases>  then per case:  <n_gens> <n_extra> <has_scale> <runs>  then runs x (<k> <count>): the round counts in the caller's order
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ipa_mixed_plan_host.hpp"

template <class T>
static void print_list(const char *name, const std::vector<T> &v) {
  printf(", \"%s\": [", name);
  for (size_t i = 0; i < v.size(); i++) printf(i ? ", %llu" : "%llu", (unsigned long long)v[i]);
  printf("]");
}

int main() {
  unsigned cases;
  if (scanf("%u", &cases) != 1) return 2;
  const BpmiOptions opt;
  for (unsigned c = 0; c < cases; c++) {
    unsigned long long n_gens, n_extra;
    unsigned runs;
    int hs;
    if (scanf("%llu %llu %d %u", &n_gens, &n_extra, &hs, &runs) != 4) return 2;
    std::vector<u32> ks;
    for (unsigned r = 0; r < runs; r++) {
      unsigned k, count;
      if (scanf("%u %u", &k, &count) != 2 || ks.size() + (size_t)count > (1u << 17)) return 2;
      ks.insert(ks.end(), count, k);
    }
    const IpamPlan p = ipa_mixed_plan(opt, n_gens, ks.size(), ks.data(), n_extra, hs);
    printf("{\"err\": %d, \"msg\": ", p.err);
    if (p.msg) printf("\"%s\"", p.msg); else printf("null");           // (the plan's texts hold no quote or backslash)
    if (!p.err) {
      printf(", \"K\": %u, \"k_top\": %u, \"n_top\": %llu, \"work\": %llu, \"waves\": %llu, \"tab_entries\": %llu, \"rec_words\": %llu", p.K, p.k_top,
             (unsigned long long)p.n_top, (unsigned long long)p.work, (unsigned long long)p.waves, (unsigned long long)p.tab_entries, (unsigned long long)p.rec_words);
      printf(", \"per_part\": %u, \"n_blocks\": %u, \"n_units\": %u, \"direct\": %d", p.per_part, p.n_blocks, p.n_units, p.direct ? 1 : 0);
      print_list("perm", p.perm);
      print_list("C", p.C);
      print_list("block_first", p.block_first);
      std::vector<u32> flat;
      for (const IpamDesc &d : p.desc) { flat.push_back(d.tab_off); flat.push_back(d.k); flat.push_back(d.kl); flat.push_back(d.rec_off); }
      print_list("desc", flat);
      flat.clear();
      for (const IpamUnit &u : p.unit) { flat.push_back(u.block); flat.push_back(u.p0); flat.push_back(u.p1); flat.push_back(u.slot); }
      print_list("units", flat);
      const char *names[12] = {"sa", "sb", "rec", "desc", "ctab", "units", "blocks", "tab", "part", "expt", "exsc", "scale"};
      const uint64_t offs[12] = {p.o_sa, p.o_sb, p.o_rec, p.o_desc, p.o_ctab, p.o_units, p.o_blocks, p.o_tab, p.o_part, p.o_expt, p.o_exsc, p.o_scale};
      const uint64_t lens[12] = {p.b_sa, p.b_sb, p.b_rec, p.b_desc, p.b_ctab, p.b_units, p.b_blocks, p.b_tab, p.b_part, p.b_expt, p.b_exsc, p.b_scale};
      printf(", \"regions\": {");
      for (int i = 0; i < 12; i++) printf("%s\"%s\": [%llu, %llu]", i ? ", " : "", names[i], (unsigned long long)offs[i], (unsigned long long)lens[i]);
      printf("}, \"total_bytes\": %llu, \"msm_pairs\": %llu, \"simds\": %u, \"threads\": %u", (unsigned long long)p.total_bytes, (unsigned long long)p.msm_pairs,
             IPAB_SIMDS, IPAB_THREADS);
      if (runs == 1) {
        const IpabPlan b = ipa_batch_plan(opt, p.n_top, ks.size(), n_extra, hs);
        if (!b.err) printf(", \"batch\": {\"per_part\": %u, \"parts\": %u, \"direct\": %d}", b.per_part, b.parts, b.direct ? 1 : 0);
      }
    }
    printf("}\n");
  }
  return 0;
}
