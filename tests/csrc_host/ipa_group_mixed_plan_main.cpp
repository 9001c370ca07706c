// ipa_group_mixed_plan_main.cpp -- the plan of bpmi_ipa_group_values_packed_mixed_dev
// (python-bulletproofs_amd/csrc/ipa_group_mixed_plan_host.hpp) printed as JSON, one line per case: tests/test_ipa_group_mixed_plan_cpu.py
// compiles this with the host compiler and checks the lines.
//   ipa_group_mixed_plan_main <case> [<case> ...]
//   case = K,protocol,has_scale,t_budget,present,n_given,outputs,group_given;k:P:tr_len:group[:flags];...
// K, protocol, has_scale, t_budget, present, n_given and the flags of a class: as ipa_packed_mixed_plan_main.  outputs: 1 when values,
// value_off and status are given; group_given: 0 makes the `group` argument NULL; group of a class: its entry of that array.
// Beside the plan every non-empty class carries "single": what ipa_group_plan decides for that class alone with the same group, and
// "layout_ok": the class's proofs are consecutive in the sorted order of ipa_mixed_plan, in their own order, with one (k, kl) and
// tables at tab_base + j tab_stride -- the layout svb_sum_element reads.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "ipa_group_mixed_plan_host.hpp"

static std::vector<std::string> split(const std::string &s, char sep) {
  std::vector<std::string> out;
  size_t at = 0;
  for (;;) {
    const size_t e = s.find(sep, at);
    out.push_back(s.substr(at, e == std::string::npos ? e : e - at));
    if (e == std::string::npos) return out;
    at = e + 1;
  }
}
static void region(const char *name, uint64_t o, uint64_t b, bool first = false) { printf("%s\"%s\": [%llu, %llu]", first ? "" : ", ", name, (unsigned long long)o, (unsigned long long)b); }
static void list(const char *name, const std::vector<u32> &v) {
  printf(", \"%s\": [", name);
  for (size_t i = 0; i < v.size(); i++) printf("%s%u", i ? ", " : "", v[i]);
  printf("]");
}

int main(int argc, char **argv) {
  const BpmiOptions opt;
  static const uint8_t dummy[8] = {0};
  for (int a = 1; a < argc; a++) {
    const std::vector<std::string> parts = split(argv[a], ';');
    const std::vector<std::string> head = split(parts[0], ',');
    if (head.size() != 8) { fprintf(stderr, "bad case %s\n", argv[a]); return 2; }
    const unsigned K = (unsigned)strtoul(head[0].c_str(), nullptr, 10);
    const int protocol = atoi(head[1].c_str()), hs = atoi(head[2].c_str());
    const uint64_t budget = strtoull(head[3].c_str(), nullptr, 10);
    const std::string present = head[4];
    const int n_given = atoi(head[5].c_str());
    const bool outputs = atoi(head[6].c_str()) != 0, group_given = atoi(head[7].c_str()) != 0;
    const size_t listed = parts.size() - 1;
    std::vector<bpmi_ipa_packed_class> cls(listed ? listed : 1);
    std::vector<std::vector<uint64_t>> offs(listed);
    std::vector<uint64_t> group(listed ? listed : 1, 0);
    memset(cls.data(), 0, sizeof(bpmi_ipa_packed_class) * cls.size());
    for (size_t c = 0; c < listed; c++) {
      const std::vector<std::string> f = split(parts[c + 1], ':');
      if (f.size() < 4) return 2;
      const std::string flags = f.size() > 4 ? f[4] : "";
      auto has = [&](char ch) {
        const char up = (char)(ch - 'a' + 'A');
        if (flags.find(up) != std::string::npos) return true;
        return present.find(ch) != std::string::npos && flags.find(ch) == std::string::npos;
      };
      bpmi_ipa_packed_class &k = cls[c];
      k.k = (uint32_t)strtoul(f[0].c_str(), nullptr, 10);
      k.n_proofs = strtoull(f[1].c_str(), nullptr, 10);
      const uint64_t tr_len = strtoull(f[2].c_str(), nullptr, 10);
      group[c] = strtoull(f[3].c_str(), nullptr, 10);
      if (k.n_proofs && k.n_proofs <= IPAB_PROOFS_MAX) {
        offs[c].resize(k.n_proofs + 1);
        for (uint64_t i = 0; i <= k.n_proofs; i++) offs[c][i] = 100 * c + i * tr_len;
        if (flags.find('D') != std::string::npos) { offs[c][0] = 5; offs[c][1] = 4; }
      } else {
        offs[c].resize(1);
      }
      if (!k.n_proofs) continue;                        // an empty class: its pointers stay NULL and are not read
      k.ab = has('a') ? dummy : nullptr; k.xs = has('x') ? dummy : nullptr; k.LR = has('l') ? dummy : nullptr; k.transcripts = has('t') ? dummy : nullptr;
      k.tr_off = has('o') ? offs[c].data() : nullptr; k.start = has('s') ? (const uint32_t *)dummy : nullptr;
      k.u = has('u') ? dummy : nullptr; k.P = has('p') ? dummy : nullptr; k.c = has('c') ? dummy : nullptr; k.head = has('h') ? dummy : nullptr;
    }
    const uint8_t *weights = present.find('w') != std::string::npos ? dummy : nullptr, *seed = present.find('d') != std::string::npos ? dummy : nullptr;
    const uint32_t n_classes = n_given < 0 ? (uint32_t)listed : (uint32_t)n_given;
    const IpagmPlan p = ipa_group_mixed_plan(opt, K, protocol, n_classes, listed ? cls.data() : nullptr, group_given ? group.data() : nullptr, weights, seed, hs, outputs, budget);
    printf("{\"err\": %d, \"msg\": ", p.err);
    if (p.err) printf("\"%s\"", p.msg.c_str()); else printf("null");           // (the plan's texts hold no quote or backslash)
    printf(", \"empty\": %d", p.empty ? 1 : 0);
    if (!p.err) {
      printf(", \"value_off\": [");
      for (size_t i = 0; i < p.value_off.size(); i++) printf("%s%llu", i ? ", " : "", (unsigned long long)p.value_off[i]);
      printf("]");
    }
    if (!p.err && !p.empty) {
      const IpapmPlan &mp = p.packed;
      const IpamPlan &b = mp.base;
      printf(", \"ngroups\": %u, \"W\": %u, \"n_blocks\": %u, \"rows_total\": %llu, \"packed_total\": %llu, \"total_bytes\": %llu, \"n_top\": %llu", p.ngroups, p.W, p.n_blocks,
             (unsigned long long)p.rows_total, (unsigned long long)mp.total_bytes, (unsigned long long)p.total_bytes, (unsigned long long)b.n_top);
      printf(", \"packed_regions\": {");
      region("sa", b.o_sa, b.b_sa, true); region("sb", b.o_sb, b.b_sb); region("rec", b.o_rec, b.b_rec); region("desc", b.o_desc, b.b_desc);
      region("ctab", b.o_ctab, b.b_ctab); region("units", b.o_units, b.b_units); region("blocks", b.o_blocks, b.b_blocks); region("tab", b.o_tab, b.b_tab);
      region("part", b.o_part, b.b_part); region("expt", b.o_expt, b.b_expt); region("exsc", b.o_exsc, b.b_exsc); region("scale", b.o_scale, b.b_scale);
      region("status", mp.o_status, mp.b_status); region("unit_table", mp.o_units, mp.b_units); region("fin", mp.o_fin, mp.b_fin); region("pairoff", mp.o_pairoff, mp.b_pairoff);
      printf("}, \"regions\": {");
      region("gsa", p.o_gsa, p.b_gsa, true); region("gsb", p.o_gsb, p.b_gsb); region("E", p.o_E, p.b_E); region("vals", p.o_vals, p.b_vals);
      region("class_tab", p.o_ctab, p.b_ctab); region("group_tab", p.o_gtab, p.b_gtab); region("light", p.o_light, p.b_light); region("mid", p.o_mid, p.b_mid);
      printf("}");
      list("class_tab", p.class_tab); list("group_tab", p.group_tab); list("light", p.light); list("mid", p.mid); list("run", p.run);
      printf(", \"rounds\": %llu, \"classes\": [", (unsigned long long)mp.round.size());
      for (uint32_t c = 0; c < n_classes; c++) {
        const IpagmClass &q = p.cls[c];
        const IpapmClass &m = mp.cls[c];
        printf("%s{\"k\": %u, \"kl\": %u, \"per\": %u, \"count\": %u, \"group\": %u, \"ngroups\": %u, \"first_group\": %u, \"pairs\": %llu, \"route\": %u, \"tab_base\": %u, "
               "\"tab_stride\": %u, \"row_off\": %u, \"block_start\": %u, \"rows\": %llu, \"extra_off\": %llu, \"gbase\": %llu, \"first_sorted\": %u, \"prep_rows\": %u",
               c ? ", " : "", q.k, q.kl, q.per, q.count, q.group, q.ngroups, q.first_group, (unsigned long long)q.pairs, q.route, q.tab_base, q.tab_stride, q.row_off, q.block_start,
               (unsigned long long)q.rows, (unsigned long long)q.extra_off, (unsigned long long)m.gbase, m.first_sorted, m.rows);
        if (q.count) {
          bool ok = true;
          for (u32 j = 0; j < q.count; j++) {
            const IpamDesc &d = b.desc[m.first_sorted + j];
            ok = ok && b.perm[m.first_sorted + j] == m.gbase + j && d.k == q.k && d.kl == q.kl && d.tab_off == q.tab_base + j * q.tab_stride;
          }
          const IpagPlan s = ipa_group_plan(opt, 1ull << q.k, protocol, q.count, ipapm_class_in(cls[c], weights, seed), hs, group[c], true, budget);
          printf(", \"layout_ok\": %d, \"single\": {\"err\": %d, \"group\": %u, \"ngroups\": %u, \"per\": %u, \"pairs\": %llu, \"route\": %u, \"b_gsa\": %llu, \"b_gsb\": %llu, \"b_E\": %llu, "
                 "\"b_vals\": %llu}", ok ? 1 : 0, s.err, s.group, s.ngroups, s.per, (unsigned long long)s.pairs, s.route, (unsigned long long)s.b_gsa, (unsigned long long)s.b_gsb,
                 (unsigned long long)s.b_E, (unsigned long long)s.b_vals);
        }
        printf("}");
      }
      printf("]");
    }
    printf("}\n");
  }
  return 0;
}
