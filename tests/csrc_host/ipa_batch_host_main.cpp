// ipa_batch_host_main.cpp -- the per-thread bodies of the batch s-vector kernels (python-bulletproofs_amd/csrc/svector_batch.hpp) built
// for the host and run the way the three kernels run them: every table record of every proof, every element of every range, then the
// finish.  tests/test_ipa_batch_host_cpu.py compiles this with the host compiler and compares the lines with Python integers.
// Input (standard input, whitespace separated; scalars as 64 hex digits, most significant first):
//   <cases>  then per case:  <k> <proofs> <parts> <has_scale>   per proof: k x (x, x^-1), a, b, w    [n scale values]
// Output: one JSON line per case: {"tab": [...], "sa": [...], "sb": [...]}, tab = per proof its records as (first, second) pairs.
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
    unsigned k, proofs, parts, has_scale;
    if (scanf("%u %u %u %u", &k, &proofs, &parts, &has_scale) != 4 || k > 16 || !proofs || !parts || parts > proofs) return 2;
    const u32 kl = k / 2, n = 1u << k, ntab = (1u << kl) + (1u << (k - kl)), rec_words = 16 * k + 24;
    std::vector<u32> recs((size_t)rec_words * proofs), scale(has_scale ? 8 * (size_t)n : 0);
    for (size_t i = 0; i < recs.size() / 8; i++) if (!read_scalar(&recs[8 * i])) return 2;
    for (size_t i = 0; i < scale.size() / 8; i++) if (!read_scalar(&scale[8 * i])) return 2;
    // k_sc_svector_tables_batch
    std::vector<u32> tabs(16 * (size_t)ntab * proofs);
    for (u32 p = 0; p < proofs; p++)
      for (u32 t = 0; t < ntab; t++) svb_table_entry(&tabs[16 * ((size_t)ntab * p + t)], &recs[(size_t)rec_words * p], k, kl, t);
    // k_sc_svector_sum over `parts` ranges, then k_sc_svector_sum_finish -- or the sums themselves (one range, no scale)
    const u32 per_part = (proofs + parts - 1) / parts;
    if ((parts - 1) * per_part >= proofs) return 2;
    std::vector<u32> sa(8 * (size_t)n), sb(8 * (size_t)n), part(16 * (size_t)n * parts);
    const bool direct = parts == 1 && !has_scale;
    for (u32 j = 0; j < parts; j++) {
      const u32 p0 = j * per_part, p1 = p0 + per_part < proofs ? p0 + per_part : proofs;
      for (u32 i = 0; i < n; i++) {
        u32 *oa = direct ? &sa[8 * (size_t)i] : &part[16 * (size_t)n * j + 8 * (size_t)i];
        u32 *ob = direct ? &sb[8 * (size_t)i] : &part[16 * (size_t)n * j + 8 * ((size_t)n + i)];
        svb_sum_element(oa, ob, tabs.data(), ntab, kl, i, p0, p1);
      }
    }
    if (!direct)
      for (u32 i = 0; i < n; i++) svb_finish_element(&sa[8 * (size_t)i], &sb[8 * (size_t)i], part.data(), parts, n, has_scale ? scale.data() : nullptr, i);
    printf("{");
    print_scalars("tab", tabs, false);
    print_scalars("sa", sa, false);
    print_scalars("sb", sb, true);
    printf("}\n");
  }
  return 0;
}
