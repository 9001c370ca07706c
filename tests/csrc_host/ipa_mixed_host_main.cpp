// ipa_mixed_host_main.cpp -- the per-thread bodies of the s-vector kernels of a batch of proofs of different lengths
// (python-bulletproofs_amd/csrc/svector_mixed.hpp) built for the host and run the way the three kernels run them, over the plan of
// ipa_mixed_plan_host.hpp: every table record of every proof, every lane of every unit, then the finish.  The partial sums start as
// 0xFF bytes: a lane that no proof of its unit covers must WRITE its zeros.  tests/test_ipa_mixed_host_cpu.py compiles this with the
// host compiler and compares the lines with Python integers.
// Input (standard input, whitespace separated; scalars as 64 hex digits, most significant first):
//   <cases>  then per case:  <n_gens> <proofs> <has_scale>   the proofs' k   per proof, the caller's order: k x (x, x^-1), a, b, w
//            [n_gens scale values]
// Output: one JSON line per case: {"n_top": .., "units": .., "per_part": .., "direct": .., "sa": [...], "sb": [...]}.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ipa_mixed_plan_host.hpp"
#include "svector_mixed.hpp"
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
  const BpmiOptions opt;
  for (unsigned c = 0; c < cases; c++) {
    unsigned long long n_gens;
    unsigned proofs, has_scale;
    if (scanf("%llu %u %u", &n_gens, &proofs, &has_scale) != 3 || !proofs || proofs > 4096) return 2;
    std::vector<u32> ks(proofs);
    for (u32 &k : ks) if (scanf("%u", &k) != 1 || k > 17) return 2;
    const IpamPlan pl = ipa_mixed_plan(opt, n_gens, proofs, ks.data(), 0, has_scale ? 2 : 0);
    if (pl.err) { fprintf(stderr, "%s\n", pl.msg); return 2; }
    // the records in SORTED order, packed; the caller's order on the input
    std::vector<std::vector<u32>> in(proofs);
    for (u32 p = 0; p < proofs; p++) {
      in[p].resize(16 * ks[p] + 24);
      for (size_t i = 0; i < in[p].size() / 8; i++) if (!read_scalar(&in[p][8 * i])) return 2;
    }
    std::vector<u32> scale(has_scale ? 8 * (size_t)n_gens : 0);
    for (size_t i = 0; i < scale.size() / 8; i++) if (!read_scalar(&scale[8 * i])) return 2;
    std::vector<u32> recs((size_t)pl.rec_words);
    for (u32 s = 0; s < proofs; s++) {
      if (pl.desc[s].rec_off + in[pl.perm[s]].size() > recs.size()) return 3;
      memcpy(&recs[pl.desc[s].rec_off], in[pl.perm[s]].data(), 4 * in[pl.perm[s]].size());
    }
    std::vector<u32> desc_words(IPAM_DESC_WORDS * (size_t)proofs);          // the bytes the device table holds
    memcpy(desc_words.data(), pl.desc.data(), 4 * desc_words.size());
    const u32 *desc = desc_words.data();
    // k_sc_svector_tables_mixed: one thread per record of the packed array; the bisection must find the proof whose table holds it
    std::vector<u32> tabs(16 * (size_t)pl.tab_entries);
    for (u32 r = 0; r < pl.tab_entries; r++) {
      const u32 s = svm_proof_of_record(desc, proofs, r);
      if (s >= proofs || pl.desc[s].tab_off > r || (s + 1 < proofs && pl.desc[s + 1].tab_off <= r)) return 3;
      svm_table_record(&tabs[16 * (size_t)r], recs.data(), desc, proofs, r);
    }
    // k_sc_svector_sum_mixed: block = unit, lane = element
    const u32 n_top = (u32)pl.n_top;
    std::vector<u32> sa(8 * (size_t)n_top), sb(8 * (size_t)n_top), part(pl.direct ? 0 : (size_t)IPAM_PART_WORDS * pl.n_units, 0xFFFFFFFFu);
    for (const IpamUnit &un : pl.unit)
      for (u32 lane = 0; lane < IPAB_THREADS; lane++) {
        const u32 i = un.block * 256u + lane;
        if (i >= n_top) continue;
        u32 *oa = pl.direct ? &sa[8 * (size_t)i] : &part[4096 * (size_t)un.slot + 8 * lane];
        u32 *ob = pl.direct ? &sb[8 * (size_t)i] : &part[4096 * (size_t)un.slot + 8 * (256 + lane)];
        svm_sum_element(oa, ob, tabs.data(), desc, pl.C.data(), i, un.p0, un.p1);
      }
    // k_sc_svector_sum_finish_mixed
    if (!pl.direct)
      for (u32 i = 0; i < n_top; i++)
        svm_finish_element(&sa[8 * (size_t)i], &sb[8 * (size_t)i], part.data(), pl.block_first.data(), has_scale ? scale.data() : nullptr, i);
    printf("{\"n_top\": %u, \"units\": %u, \"per_part\": %u, \"direct\": %d, ", n_top, pl.n_units, pl.per_part, pl.direct ? 1 : 0);
    print_scalars("sa", sa, false);
    print_scalars("sb", sb, true);
    printf("}\n");
  }
  return 0;
}
