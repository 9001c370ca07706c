// rp_group_mixed_plan_main.cpp -- the plan of bpmi_rp_batch_group_values_mixed_dev (python-bulletproofs_amd/csrc/rp_group_mixed_plan_host.hpp)
// printed as one JSON line: tests/test_rp_group_mixed_plan_cpu.py compiles this with the host compiler and checks the line.
//   rp_group_mixed_plan_main <rp_overlap> <n_gens_max> <present> <class> ...
//   rp_group_mixed_plan_main route <pairs>                     the route of a class whose full group has that many pairs
// present: one letter per argument that is NOT NULL, among c(lasses) w(eights) d (seed) o(thers: d_gens, d_points, d_scalars) g(roup)
// r(esults: values, value_off, status);
// class: n_gens:values_per_proof:n_proofs:group:present with present among b(lobs) o(ffsets) v(_points).  Every proof is empty (all
// offsets zero): the plan reads the offset tables and the first proof's format byte, nothing else.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "rp_group_mixed_plan_host.hpp"

static void region(const char *name, const RpRegion &r) { printf(", \"%s\": [%zu, %zu]", name, r.off, r.bytes); }
static void list(const char *name, const std::vector<u32> &v) {
  printf(", \"%s\": [", name);
  for (size_t i = 0; i < v.size(); i++) printf("%s%u", i ? ", " : "", v[i]);
  printf("]");
}

int main(int argc, char **argv) {
  if (argc == 3 && !strcmp(argv[1], "route")) { printf("{\"route\": %d}\n", (int)rp_group_route(strtoull(argv[2], nullptr, 10))); return 0; }
  if (argc < 4) { fprintf(stderr, "usage: %s rp_overlap n_gens_max present class ...\n", argv[0]); return 2; }
  BpmiOptions opt;
  opt.opt_rp_overlap = atoi(argv[1]);
  const unsigned n_gens_max = (unsigned)strtoul(argv[2], nullptr, 10);
  const char *present = argv[3];
  const int given = argc - 4;
  static const uint8_t dummy[8] = {0};
  std::vector<bpmi_rp_class> cls(given > 0 ? given : 1);
  std::vector<uint64_t> group(cls.size(), 0);
  std::vector<std::vector<uint64_t>> offs(cls.size());
  memset(cls.data(), 0, sizeof(bpmi_rp_class) * cls.size());
  for (int c = 0; c < given; c++) {
    unsigned n = 0, m = 0;
    unsigned long long np = 0, grp = 0;
    char have[16] = {0};
    if (sscanf(argv[4 + c], "%u:%u:%llu:%llu:%15s", &n, &m, &np, &grp, have) < 4) { fprintf(stderr, "bad class %s\n", argv[4 + c]); return 2; }
    const unsigned long long table = np <= (1ull << 22) ? np : 0;
    offs[c].assign(table + 1, 0);
    cls[c].n_gens = n; cls[c].values_per_proof = m; cls[c].n_proofs = np; group[c] = grp;
    cls[c].blobs = strchr(have, 'b') ? dummy : nullptr; cls[c].blobs_len = 0;
    cls[c].blob_off = strchr(have, 'o') ? offs[c].data() : nullptr;
    cls[c].v_points = strchr(have, 'v') ? dummy : nullptr;
  }
  const RpgmPlan p = rp_group_mixed_plan(opt, (uint32_t)given, strchr(present, 'c') ? cls.data() : nullptr, n_gens_max, strchr(present, 'g') ? group.data() : nullptr,
                                         strchr(present, 'w') != nullptr, strchr(present, 'd') != nullptr, strchr(present, 'o') != nullptr, strchr(present, 'r') != nullptr);
  printf("{\"err\": %d, \"msg\": \"%s\"", p.err, p.msg.c_str());           // (the plan's texts hold no quote or backslash)
  // what an error must leave unset is printed on errors too
  printf(", \"ngroups\": %u, \"W\": %u, \"need\": %zu, \"pin_bytes\": %zu, \"gfin_base\": %zu, \"copies_base\": %zu, \"mixed_need\": %zu, \"mixed_n_classes\": %u, \"n_proofs\": %llu",
         p.ngroups, p.W, p.need, p.pin_bytes, p.gfin_base, p.copies_base, p.mixed.need, p.mixed.n_classes, (unsigned long long)p.mixed.n_proofs);
  region("verdict", p.verdict); region("E", p.E); region("vals", p.vals); region("gtab", p.gtab); region("light_list", p.light_list); region("mid_list", p.mid_list);
  list("group_tab", p.group_tab); list("light", p.light); list("mid", p.mid); list("run", p.run);
  printf(", \"value_off\": [");
  for (size_t i = 0; i < p.value_off.size(); i++) printf("%s%llu", i ? ", " : "", (unsigned long long)p.value_off[i]);
  printf("], \"copies\": [");
  for (size_t i = 0; i < p.copies.size(); i++) printf("%s{\"n\": %u, \"pts_off\": %u, \"at\": [%zu, %zu]}", i ? ", " : "", p.copies[i].n, p.copies[i].pts_off, p.copies[i].at.off, p.copies[i].at.bytes);
  printf("], \"classes\": [");
  for (size_t c = 0; c < p.cls.size(); c++) {
    const RpgmClass &q = p.cls[c];
    const RpMixedClass &mc = p.mixed.cls[c];
    printf("%s{\"n\": %u, \"m\": %u, \"per\": %u, \"count\": %u, \"group\": %u, \"ngroups\": %u, \"first_group\": %u, \"pairs\": %llu, \"route\": %d, \"gens_off\": %u, \"gfin_word\": %u, "
           "\"o_verdict\": %zu, \"first\": %llu, \"pair_off\": %llu, \"nv\": %llu, \"decode\": %d",
           c ? ", " : "", q.n, q.m, q.per, q.count, q.group, q.ngroups, q.first_group, (unsigned long long)q.pairs, (int)q.route, q.gens_off, q.gfin_word, q.o_verdict,
           (unsigned long long)mc.first, (unsigned long long)mc.pair_off, (unsigned long long)mc.nv, (int)mc.pl.decode);
    region("gsum", q.gsum); region("gfin", q.gfin); region("ptflag", q.ptflag);
    printf("}");
  }
  printf("]}\n");
  return 0;
}
