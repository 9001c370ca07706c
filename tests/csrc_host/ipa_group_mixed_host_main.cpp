// ipa_group_mixed_host_main.cpp -- the per-thread body of the grouped s-vector sum over classes of different lengths
// (svm_group_row_element, python-bulletproofs_amd/csrc/svector_mixed.hpp) built for the host and run the way
// k_sc_svector_sum_groups_mixed runs it, over the tables of the real plan (ipa_group_mixed_plan_host.hpp): the classes' records at the
// offsets of the mixed plan (descending k), every record of the packed half-table array by svm_table_record, then every lane of every
// block of the launch with the plan's class table.  tests/test_ipa_group_mixed_host_cpu.py compiles this with the host compiler and
// compares the lines with Python integers.
// Input (standard input, whitespace separated; scalars as 64 hex digits, most significant first):
//   <cases>  then per case:  <classes> <has_scale>   per class: <k> <proofs> <group>
//                            per class, per proof: k x (x, x^-1), a, b, w      [n_top scale values]
// Output: one JSON line per case: {"classes": [{"sa": [...], "sb": [...]}, ...], "pad_untouched": 0 | 1} -- per class the rows of its
// groups one after the other, n values each; pad_untouched: no scalar outside the classes' rows was written.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ipa_group_mixed_plan_host.hpp"
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
static void print_scalars(const char *name, const u32 *v, size_t count, bool last) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < count; i++) {
    printf(i ? ", \"" : "\"");
    for (int q = 7; q >= 0; q--) printf("%08x", v[8 * i + q]);
    printf("\"");
  }
  printf(last ? "]" : "], ");
}

int main() {
  static const uint8_t dummy[8] = {0};
  const BpmiOptions opt;
  unsigned cases;
  if (scanf("%u", &cases) != 1) return 2;
  for (unsigned cs = 0; cs < cases; cs++) {
    unsigned n_classes, has_scale;
    if (scanf("%u %u", &n_classes, &has_scale) != 2 || !n_classes || n_classes > 8) return 2;
    std::vector<bpmi_ipa_packed_class> cls(n_classes);
    std::vector<std::vector<uint64_t>> offs(n_classes);
    std::vector<uint64_t> group(n_classes);
    memset(cls.data(), 0, sizeof(bpmi_ipa_packed_class) * n_classes);
    u32 K = 0;
    for (unsigned c = 0; c < n_classes; c++) {
      unsigned k, proofs, g;
      if (scanf("%u %u %u", &k, &proofs, &g) != 3 || k > 12 || !proofs || proofs > 4096) return 2;
      bpmi_ipa_packed_class &q = cls[c];
      q.k = k; q.n_proofs = proofs; group[c] = g;
      offs[c].assign(proofs + 1, 0);
      for (unsigned i = 0; i <= proofs; i++) offs[c][i] = 50ull * i;
      q.ab = q.transcripts = q.u = q.P = dummy; q.xs = q.LR = k ? dummy : nullptr; q.tr_off = offs[c].data();
      if (k > K) K = k;
    }
    const IpagmPlan gp = ipa_group_mixed_plan(opt, K, 2, n_classes, cls.data(), group.data(), nullptr, dummy, has_scale ? 1 : 0, true, 0);
    if (gp.err) { fprintf(stderr, "plan: %s\n", gp.msg.c_str()); return 2; }
    const IpamPlan &bp = gp.packed.base;
    std::vector<u32> recs((size_t)bp.rec_words), scale(has_scale ? 8 * (size_t)bp.n_top : 0);
    for (unsigned c = 0; c < n_classes; c++) {
      const size_t words = (size_t)(16 * cls[c].k + 24) * cls[c].n_proofs;
      for (size_t i = 0; i < words / 8; i++) if (!read_scalar(&recs[gp.packed.cls[c].rec_off + 8 * i])) return 2;
    }
    for (size_t i = 0; i < scale.size() / 8; i++) if (!read_scalar(&scale[8 * i])) return 2;
    // k_sc_svector_tables_mixed
    std::vector<u32> desc;
    for (const IpamDesc &d : bp.desc) { desc.push_back(d.tab_off); desc.push_back(d.k); desc.push_back(d.kl); desc.push_back(d.rec_off); }
    std::vector<u32> tabs(16 * (size_t)bp.tab_entries);
    for (u32 r = 0; r < (u32)bp.tab_entries; r++) svm_table_record(&tabs[16 * (size_t)r], recs.data(), desc.data(), (u32)bp.n_proofs, r);
    // k_sc_svector_sum_groups_mixed: every lane of every block; the rows start out as a pattern no scalar has
    const size_t padded = 256 * (size_t)gp.n_blocks;
    std::vector<u32> sa(8 * padded, 0xFFFFFFFFu), sb(8 * padded, 0xFFFFFFFFu);
    std::vector<char> written(padded, 0);
    const u32 n_cls = (u32)(gp.class_tab.size() / IPAGM_CLASS_WORDS);
    for (u32 b = 0; b < gp.n_blocks; b++)
      for (u32 lane = 0; lane < 256; lane++) {
        u32 ra[8], rb[8], idx = 0;
        if (!svm_group_row_element(ra, rb, idx, tabs.data(), gp.class_tab.data(), n_cls, has_scale ? scale.data() : nullptr, b, lane)) continue;
        if (idx >= padded || written[idx]) { fprintf(stderr, "block %u lane %u: scalar %u out of range or written twice\n", b, lane, idx); return 3; }
        written[idx] = 1;
        memcpy(&sa[8 * (size_t)idx], ra, 32);
        memcpy(&sb[8 * (size_t)idx], rb, 32);
      }
    bool pad_ok = true;
    std::vector<char> owned(padded, 0);
    for (unsigned c = 0; c < n_classes; c++)
      for (uint64_t i = 0; i < gp.cls[c].rows; i++) owned[gp.cls[c].row_off + i] = 1;
    for (size_t i = 0; i < padded; i++) pad_ok = pad_ok && written[i] == owned[i];
    printf("{\"classes\": [");
    for (unsigned c = 0; c < n_classes; c++) {
      printf(c ? ", {" : "{");
      print_scalars("sa", &sa[8 * (size_t)gp.cls[c].row_off], (size_t)gp.cls[c].rows, false);
      print_scalars("sb", &sb[8 * (size_t)gp.cls[c].row_off], (size_t)gp.cls[c].rows, true);
      printf("}");
    }
    printf("], \"pad_untouched\": %d}\n", pad_ok ? 1 : 0);
  }
  return 0;
}
