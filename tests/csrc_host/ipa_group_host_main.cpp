// ipa_group_host_main.cpp -- the per-thread body of the grouped s-vector sum (svb_group_element, python-bulletproofs_amd/csrc/svector_batch.hpp)
// built for the host and run the way k_sc_svector_sum_groups runs it: the half tables of every proof, then one flat index over
// (group, element) -- t = idx >> k, i = idx & (n - 1).  tests/test_ipa_group_host_cpu.py compiles this with the host compiler and compares
// the lines with Python integers.
// Input (standard input, whitespace separated; scalars as 64 hex digits, most significant first):
//   <cases>  then per case:  <k> <proofs> <group> <has_scale>   per proof: k x (x, x^-1), a, b, w    [n scale values]
// Output: one JSON line per case: {"sa": [...], "sb": [...]}, the rows of the groups one after the other, n values each.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "svector_batch.hpp"
using namespace bpmi;

static bool read_scalar(u32 w[8]) {
  char s[80];
  if (scanf("%79s", s) != 1 || strlen(s) != 64) return false;
  for (int i = 0; i < 8; i++) {
    char part[9];
    memcpy(part, s + 8 * (7 - i), 8);
    part[8] = 0;
    w[i] = (u32)strtoul(part, nullptr, 16);
  }
  return true;
}
static void print_scalars(const char *name, const std::vector<u32> &v, bool last) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size() / 8; i++) {
    printf(i ? ", \"" : "\"");
    for (int q = 7; q >= 0; q--) printf("%08x", v[8 * i + q]);
    printf("\"");
  }
  printf(last ? "]" : "], ");
}

int main() {
  unsigned cases;
  if (scanf("%u", &cases) != 1) return 2;
  for (unsigned c = 0; c < cases; c++) {
    unsigned k, proofs, group, has_scale;
    if (scanf("%u %u %u %u", &k, &proofs, &group, &has_scale) != 4 || k > 16 || !proofs || !group || group > proofs) return 2;
    const u32 kl = k / 2, n = 1u << k, ntab = (1u << kl) + (1u << (k - kl)), rec_words = 16 * k + 24;
    std::vector<u32> recs((size_t)rec_words * proofs), scale(has_scale ? 8 * (size_t)n : 0);
    for (size_t i = 0; i < recs.size() / 8; i++) if (!read_scalar(&recs[8 * i])) return 2;
    for (size_t i = 0; i < scale.size() / 8; i++) if (!read_scalar(&scale[8 * i])) return 2;
    // k_sc_svector_tables_batch
    std::vector<u32> tabs(16 * (size_t)ntab * proofs);
    for (u32 p = 0; p < proofs; p++)
      for (u32 t = 0; t < ntab; t++) svb_table_entry(&tabs[16 * ((size_t)ntab * p + t)], &recs[(size_t)rec_words * p], k, kl, t);
    // k_sc_svector_sum_groups
    const u32 ngroups = (proofs + group - 1) / group;
    std::vector<u32> sa(8 * (size_t)n * ngroups), sb(8 * (size_t)n * ngroups);
    for (u32 idx = 0; idx < ngroups * n; idx++) {
      const u32 t = idx >> k, i = idx & (n - 1u);
      svb_group_element(&sa[8 * (size_t)idx], &sb[8 * (size_t)idx], tabs.data(), ntab, kl, i, t, group, proofs, has_scale ? scale.data() : nullptr);
    }
    printf("{");
    print_scalars("sa", sa, false);
    print_scalars("sb", sb, true);
    printf("}\n");
  }
  return 0;
}
