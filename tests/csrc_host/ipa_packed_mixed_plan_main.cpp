// ipa_packed_mixed_plan_main.cpp -- the plan of a batch of packed inner-product proofs of different lengths
// (python-bulletproofs_amd/csrc/ipa_packed_mixed_plan_host.hpp) printed as JSON, one line per case: tests/test_ipa_packed_mixed_plan_cpu.py
// compiles this with the host compiler and checks the lines.
//   ipa_packed_mixed_plan_main <case> [<case> ...]
//   case = K,protocol,has_scale,t_budget,present,n_given;k:P:tr_len[:flags];k:P:tr_len[:flags];...
// present: as ipa_packed_plan_main, one letter per array that is NOT NULL in every class -- a(b) x(s) l(LR) t(ranscripts) o(tr_off) s(tart)
// u p(P) c h(ead) -- plus w (weights) / d (seed) for the call; n_given: the n_classes argument (-1: the number of classes listed; with no
// class listed the classes pointer is NULL); flags of one class: a lower-case letter makes that array NULL in this class, an upper-case
// one (C, H, S) makes it non-NULL in this class only, "D" makes its tr_off decrease.  The arrays other than tr_off are never read by the
// plan: they are dummy non-NULL addresses.  The single-class plan of every non-empty class is printed beside it ("single").
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "ipa_packed_mixed_plan_host.hpp"

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

int main(int argc, char **argv) {
  const BpmiOptions opt;
  static const uint8_t dummy[8] = {0};
  for (int a = 1; a < argc; a++) {
    const std::vector<std::string> parts = split(argv[a], ';');
    const std::vector<std::string> head = split(parts[0], ',');
    if (head.size() != 6) { fprintf(stderr, "bad case %s\n", argv[a]); return 2; }
    const unsigned K = (unsigned)strtoul(head[0].c_str(), nullptr, 10);
    const int protocol = atoi(head[1].c_str()), hs = atoi(head[2].c_str());
    const uint64_t budget = strtoull(head[3].c_str(), nullptr, 10);
    const std::string present = head[4];
    const int n_given = atoi(head[5].c_str());
    const size_t listed = parts.size() - 1;
    std::vector<bpmi_ipa_packed_class> cls(listed ? listed : 1);
    std::vector<std::vector<uint64_t>> offs(listed);
    memset(cls.data(), 0, sizeof(bpmi_ipa_packed_class) * cls.size());
    for (size_t c = 0; c < listed; c++) {
      const std::vector<std::string> f = split(parts[c + 1], ':');
      if (f.size() < 3) return 2;
      const std::string flags = f.size() > 3 ? f[3] : "";
      auto has = [&](char ch) {
        const char up = (char)(ch - 'a' + 'A');
        if (flags.find(up) != std::string::npos) return true;
        return present.find(ch) != std::string::npos && flags.find(ch) == std::string::npos;
      };
      bpmi_ipa_packed_class &k = cls[c];
      k.k = (uint32_t)strtoul(f[0].c_str(), nullptr, 10);
      k.n_proofs = strtoull(f[1].c_str(), nullptr, 10);
      const uint64_t tr_len = strtoull(f[2].c_str(), nullptr, 10);
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
    const IpapmPlan p = ipa_packed_mixed_plan(opt, K, protocol, n_classes, listed ? cls.data() : nullptr, weights, seed, hs, budget);
    printf("{\"err\": %d, \"msg\": ", p.err);
    if (p.err) printf("\"%s\"", p.msg.c_str()); else printf("null");           // (the plan's texts hold no quote or backslash)
    printf(", \"empty\": %d", p.empty ? 1 : 0);
    if (!p.err && !p.empty) {
      const IpamPlan &b = p.base;
      printf(", \"n_proofs\": %llu, \"n_extra\": %llu, \"n_top\": %llu, \"rec_words\": %llu, \"base_total\": %llu, \"total_bytes\": %llu, \"tr_bytes\": %llu",
             (unsigned long long)b.n_proofs, (unsigned long long)b.n_extra, (unsigned long long)b.n_top, (unsigned long long)b.rec_words,
             (unsigned long long)b.total_bytes, (unsigned long long)p.total_bytes, (unsigned long long)p.tr_bytes);
      printf(", \"perm_k\": [");
      for (size_t s = 0; s < b.perm.size(); s++) printf("%s%u", s ? ", " : "", b.desc[s].k);
      printf("], \"base_regions\": {");
      region("sa", b.o_sa, b.b_sa, true); region("sb", b.o_sb, b.b_sb); region("rec", b.o_rec, b.b_rec); region("desc", b.o_desc, b.b_desc);
      region("ctab", b.o_ctab, b.b_ctab); region("units", b.o_units, b.b_units); region("blocks", b.o_blocks, b.b_blocks); region("tab", b.o_tab, b.b_tab);
      region("part", b.o_part, b.b_part); region("expt", b.o_expt, b.b_expt); region("exsc", b.o_exsc, b.b_exsc); region("scale", b.o_scale, b.b_scale);
      printf("}, \"regions\": {");
      region("status", p.o_status, p.b_status, true); region("unit_table", p.o_units, p.b_units); region("fin", p.o_fin, p.b_fin); region("pairoff", p.o_pairoff, p.b_pairoff);
      printf("}, \"classes\": [");
      for (uint32_t c = 0; c < p.n_classes; c++) {
        const IpapmClass &m = p.cls[c];
        printf("%s{\"k\": %u, \"pairs\": %u, \"n_proofs\": %llu, \"gbase\": %llu, \"first_sorted\": %u, \"rec_off\": %u, \"extra_off\": %llu, \"W\": %u, \"rows\": %u, \"chunks\": %u, \"regions\": {",
               c ? ", " : "", m.k, m.pairs, (unsigned long long)m.n_proofs, (unsigned long long)m.gbase, m.first_sorted, m.rec_off, (unsigned long long)m.extra_off, m.W, m.rows, m.chunks);
        region("ab", m.o_ab, m.b_ab, true); region("xs", m.o_xs, m.b_xs); region("lr", m.o_lr, m.b_lr); region("tr", m.o_tr, m.b_tr); region("troff", m.o_troff, m.b_troff);
        region("start", m.o_start, m.b_start); region("u", m.o_u, m.b_u); region("P", m.o_P, m.b_P); region("c", m.o_c, m.b_c); region("head", m.o_head, m.b_head);
        region("w", m.o_w, m.b_w); region("roles", m.o_roles, m.b_roles); region("T", m.o_T, m.b_T);
        printf("}");
        if (m.n_proofs) {                               // what ipa_packed_plan lays out for this class alone
          const IpapPlan s = ipa_packed_plan(opt, m.k, protocol, m.n_proofs, ipapm_class_in(cls[c], weights, seed), hs);
          printf(", \"single\": {\"base_total\": %llu, \"rec_words\": %u, \"pairs\": %u, \"W\": %u, \"rows\": %u, \"total_bytes\": %llu, \"regions\": {", (unsigned long long)s.base.total_bytes,
                 s.base.rec_words, s.pairs, s.W, s.rows, (unsigned long long)s.total_bytes);
          region("ab", s.o_ab, s.b_ab, true); region("xs", s.o_xs, s.b_xs); region("lr", s.o_lr, s.b_lr); region("tr", s.o_tr, s.b_tr); region("troff", s.o_troff, s.b_troff);
          region("start", s.o_start, s.b_start); region("u", s.o_u, s.b_u); region("P", s.o_P, s.b_P); region("c", s.o_c, s.b_c); region("head", s.o_head, s.b_head);
          region("w", s.o_w, s.b_w); region("roles", s.o_roles, s.b_roles); region("status", s.o_status, s.b_status); region("T", s.o_T, s.b_T);
          printf("}}");
        }
        printf("}");
      }
      printf("], \"units\": [");
      for (size_t i = 0; i < p.unit.size(); i++) printf("%s[%u, %u, %u]", i ? ", " : "", p.unit[i].cls, p.unit[i].chunk, p.unit[i].first_block);
      printf("], \"rounds\": [");
      for (size_t r = 0; r < p.round.size(); r++)
        printf("%s[%u, %u, %u, %u]", r ? ", " : "", p.round[r].first_unit, p.round[r].n_units, p.round[r].blocks, p.round[r].lds_bytes);
      printf("], \"fin_cls\": [");
      for (size_t j = 0; j < p.fin_cls.size(); j++) printf("%s%u", j ? ", " : "", p.fin_cls[j]);
      printf("], \"pair_off\": [");
      for (size_t j = 0; j < p.pair_off.size(); j++) printf("%s%u", j ? ", " : "", p.pair_off[j]);
      printf("]");
    }
    printf("}\n");
  }
  return 0;
}
