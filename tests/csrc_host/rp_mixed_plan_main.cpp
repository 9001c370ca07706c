// rp_mixed_plan_main.cpp -- the plan of a mixed batch of range proofs (python-bulletproofs_amd/csrc/rp_mixed_plan_host.hpp) printed as
// one JSON line: tests/test_rp_mixed_plan_cpu.py compiles this with the host compiler and checks the line.
//   rp_mixed_plan_main <rp_rows> <n_gens_max> <present> <n_classes or -1> <class> ...
// present: one letter per argument that is NOT NULL, among c(lasses) w(eights) d (seed) o(thers: d_gens, d_points, d_scalars, out, first_bad);
// n_classes: the count handed to the plan, -1 = the number of <class> arguments (so that 0 and 65 can be asked for with fewer);
// class: n_gens:values_per_proof:n_proofs:proof_len:present with present among b(lobs) o(ffsets) v(_points) and d = an offset table that
// decreases.  Every proof of a class is proof_len zero bytes; the commitments are never read by the plan.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "rp_mixed_plan_host.hpp"

int main(int argc, char **argv) {
  if (argc < 5) { fprintf(stderr, "usage: %s rp_rows n_gens_max present n_classes class ...\n", argv[0]); return 2; }
  BpmiOptions opt;
  opt.opt_rp_rows = atoi(argv[1]);
  const unsigned n_gens_max = (unsigned)strtoul(argv[2], nullptr, 10);
  const char *present = argv[3];
  const long asked = atol(argv[4]);
  const int given = argc - 5;
  static const uint8_t dummy[8] = {0};
  std::vector<bpmi_rp_class> cls(given > 0 ? given : 1);
  std::vector<std::vector<uint64_t>> offs(cls.size());
  std::vector<std::vector<uint8_t>> blobs(cls.size());
  memset(cls.data(), 0, sizeof(bpmi_rp_class) * cls.size());
  for (int c = 0; c < given; c++) {
    unsigned n = 0, m = 0;
    unsigned long long np = 0, len = 0;
    char have[16] = {0};
    if (sscanf(argv[5 + c], "%u:%u:%llu:%llu:%15s", &n, &m, &np, &len, have) < 4) { fprintf(stderr, "bad class %s\n", argv[5 + c]); return 2; }
    const unsigned long long table = np <= (1ull << 22) ? np : 0;       // (the plan refuses more proofs before it reads the table)
    offs[c].resize(table + 1);
    for (unsigned long long i = 0; i <= table; i++) offs[c][i] = i * len;
    if (strchr(have, 'd') && table >= 1) { offs[c][0] = 5; offs[c][1] = 4; }
    blobs[c].assign(table * len + 8, 0);
    cls[c].n_gens = n; cls[c].values_per_proof = m; cls[c].n_proofs = np;
    cls[c].blobs = strchr(have, 'b') ? blobs[c].data() : nullptr; cls[c].blobs_len = table * len;
    cls[c].blob_off = strchr(have, 'o') ? offs[c].data() : nullptr;
    cls[c].v_points = strchr(have, 'v') ? dummy : nullptr;
  }
  const uint32_t n_classes = asked < 0 ? (uint32_t)given : (uint32_t)asked;
  const RpMixedPlan p = rp_mixed_plan(opt, n_classes, strchr(present, 'c') ? cls.data() : nullptr, n_gens_max, strchr(present, 'w') != nullptr,
                                      strchr(present, 'd') != nullptr, strchr(present, 'o') != nullptr);
  printf("{\"err\": %d, \"msg\": \"%s\"", p.err, p.msg.c_str());           // (the plan's texts hold no quote or backslash)
  // what an error must leave unset is printed on errors too
  printf(", \"n_classes\": %u, \"N\": %u, \"n_cls\": %zu, \"n_proofs\": %llu, \"n_pairs\": %llu, \"n_v\": %llu, \"stage_bytes\": %zu, \"need\": %zu, \"pin_bytes\": %zu", p.n_classes,
         p.N, p.cls.size(), (unsigned long long)p.n_proofs, (unsigned long long)p.n_pairs, (unsigned long long)p.n_v, p.stage_bytes, p.need, p.pin_bytes);
  printf(", \"vstage\": [%zu, %llu], \"merged\": [%zu, %zu], \"bad\": [%zu, %zu], \"units\": [%zu, %zu], \"unit_stride\": %d", p.o_vstage, 64ull * p.n_v, p.merged.off,
         p.merged.bytes, p.bad.off, p.bad.bytes, p.units.off, p.units.bytes, RP_MIXED_UNIT_STRIDE);
  printf(", \"classes\": [");
  for (size_t c = 0; c < p.cls.size(); c++) {
    const RpMixedClass &m = p.cls[c];
    printf("%s{\"in\": [%zu, %zu], \"buf\": [%zu, %zu], \"first\": %llu, \"nv\": %llu, \"npts\": %llu, \"pair_off\": %llu, \"v_off\": %llu, \"chunks\": %u, \"rows\": %u, \"P\": %u, "
           "\"k\": %u, \"m\": %u, \"fmt0\": %u, \"lds\": %zu}",
           c ? ", " : "", m.in_base, m.pl.stage_bytes, m.buf_base, m.pl.need, (unsigned long long)m.first, (unsigned long long)m.nv, (unsigned long long)m.npts,
           (unsigned long long)m.pair_off, (unsigned long long)m.v_off, m.chunks, m.pl.rows, m.pl.P, m.pl.k, m.pl.m, (unsigned)m.pl.fmt0, m.pl.lds_bytes);
  }
  printf("], \"rounds\": [");
  for (size_t r = 0; r < p.round.size(); r++) {
    printf("%s{\"lds\": %zu, \"units\": [", r ? ", " : "", p.round[r].lds_bytes);
    for (u32 i = 0; i < p.round[r].n_units; i++) printf("%s[%u, %u]", i ? ", " : "", p.unit[p.round[r].first_unit + i].cls, p.unit[p.round[r].first_unit + i].chunk);
    printf("]}");
  }
  printf("], \"n_units\": %zu}\n", p.unit.size());
  return 0;
}
