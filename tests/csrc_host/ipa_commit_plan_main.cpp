// ipa_commit_plan_main.cpp -- the plan of the batched inner-product prover's statements (bpmi_ipa_batch_prover_commit_batch; the
// functions appended to python-bulletproofs_amd/csrc/ipa_prove_plan_host.hpp) printed as JSON: tests/test_ipa_commit_plan_cpu.py
// compiles this with the host compiler and checks the lines.
//   ipa_commit_plan_main errors           one line: every text of ipp_commit_error
//   ipa_commit_plan_main bases <lo> <hi>  one line per n in [lo, hi]: ipp_commit_bases of every NULL / u combination, the device copy
//                                         and its offsets, and (for a power of two) what ipp_plan still gives for that n
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ipa_prove_plan_host.hpp"

static void print_text(const char *s) {
  if (!s) { printf("null"); return; }
  printf("\"%s\"", s);                       // (the plan's texts hold no quote or backslash)
}
static void print_list(const std::vector<unsigned short> &v) {
  printf("[");
  for (size_t i = 0; i < v.size(); i++) printf(i ? ",%u" : "%u", (unsigned)v[i]);
  printf("]");
}

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "errors")) {
    // every combination of (pv, out, a, b, t) x u_mode -1 .. 3, keyed "pv out a b t mode" in 0 / 1
    printf("{");
    bool first = true;
    for (int bits = 0; bits < 32; bits++) for (int mode = -1; mode <= 3; mode++) {
      IppCommitCall c;
      c.pv = bits & 1; c.out = bits & 2; c.a = bits & 4; c.b = bits & 8; c.t = bits & 16; c.u_mode = mode;
      printf(first ? "\"%d%d%d%d%d %d\": " : ", \"%d%d%d%d%d %d\": ", (int)c.pv, (int)c.out, (int)c.a, (int)c.b, (int)c.t, mode);
      first = false;
      print_text(ipp_commit_error(c));
    }
    printf("}\n");
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "bases")) {
    const uint32_t lo = (uint32_t)strtoul(argv[2], nullptr, 10), hi = (uint32_t)strtoul(argv[3], nullptr, 10);
    for (uint32_t n = lo; n <= hi; n++) {
      printf("{\"n\": %u, \"lists\": {", n);
      bool first = true;
      for (int bits = 0; bits < 8; bits++) {
        const bool a = bits & 1, b = bits & 2, u = bits & 4;
        printf(first ? "\"%d%d%d\": " : ", \"%d%d%d\": ", (int)a, (int)b, (int)u);
        first = false;
        print_list(ipp_commit_bases(n, a, b, u));
      }
      printf("}, \"all\": ");
      print_list(ipp_commit_bases_all(n));
      printf(", \"offsets\": {\"11\": %u, \"10\": %u, \"01\": %u}", ipp_commit_bases_offset(n, true, true), ipp_commit_bases_offset(n, true, false),
             ipp_commit_bases_offset(n, false, true));
      if (!(n & (n - 1))) {
        const IppPlan p = ipp_plan(n, 0);
        printf(", \"plan\": {\"err\": %d, \"k\": %u, \"NT\": %u, \"per_block\": %u, \"nbases\": %u, \"off_head\": %u, \"off_round\": %u, \"max_proofs\": %llu, \"bases\": ",
               p.err, p.k, p.NT, p.per_block, p.nbases, p.off_head, p.off_round, (unsigned long long)p.max_proofs);
        print_list(p.bases);
        printf("}");
      }
      printf("}\n");
    }
    return 0;
  }
  fprintf(stderr, "usage: %s errors | bases <lo> <hi>\n", argv[0]);
  return 2;
}
