// ipa_group_plan_main.cpp -- the plan of bpmi_ipa_group_values_packed_dev (python-bulletproofs_amd/csrc/ipa_group_plan_host.hpp) printed as
// JSON, one line per case: tests/test_ipa_group_plan_cpu.py compiles this with the host compiler and checks the lines.
//   ipa_group_plan_main <k> <protocol> <n_proofs> <tr_len> <has_scale> <present> <offsets> <group> <outputs> <t_budget> [...]
// k, protocol, n_proofs, tr_len, has_scale, present, offsets: as ipa_packed_plan_main (n = 2^k; every transcript tr_len bytes);
// outputs: 1 when `values` and `status` are given; t_budget: bytes of one launch's transposed transcripts, 0 = the default.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ipa_group_plan_host.hpp"

int main(int argc, char **argv) {
  if (argc < 11 || (argc - 1) % 10) { fprintf(stderr, "usage: %s k protocol n_proofs tr_len has_scale present offsets group outputs t_budget ...\n", argv[0]); return 2; }
  const BpmiOptions opt;
  static const uint8_t dummy[8] = {0};
  for (int a = 1; a + 9 < argc; a += 10) {
    const unsigned k = (unsigned)strtoul(argv[a], nullptr, 10);
    const int protocol = atoi(argv[a + 1]);
    const unsigned long long np = strtoull(argv[a + 2], nullptr, 10), tr_len = strtoull(argv[a + 3], nullptr, 10);
    const int hs = atoi(argv[a + 4]);
    const char *present = argv[a + 5], *mode = argv[a + 6];
    const unsigned long long group = strtoull(argv[a + 7], nullptr, 10), budget = strtoull(argv[a + 9], nullptr, 10);
    const bool outputs = atoi(argv[a + 8]) != 0;
    auto has = [&](char ch) { return strchr(present, ch) != nullptr; };
    std::vector<uint64_t> off;
    if (np <= IPAB_PROOFS_MAX) {
      off.resize(np + 1);
      const uint64_t first = strcmp(mode, "first") == 0 ? 1000 : 0;
      for (uint64_t i = 0; i <= np; i++) off[i] = first + i * tr_len;
      if (strcmp(mode, "down") == 0 && np >= 1) { off[0] = 5; off[1] = 4; }
    } else {
      off.resize(1);
    }
    IpaPackedIn in;
    in.ab = has('a') ? dummy : nullptr; in.xs = has('x') ? dummy : nullptr; in.LR = has('l') ? dummy : nullptr; in.transcripts = has('t') ? dummy : nullptr;
    in.tr_off = has('o') ? off.data() : nullptr; in.start = has('s') ? (const uint32_t *)dummy : nullptr;
    in.u = has('u') ? dummy : nullptr; in.P = has('p') ? dummy : nullptr; in.c = has('c') ? dummy : nullptr; in.head = has('h') ? dummy : nullptr;
    in.weights = has('w') ? dummy : nullptr; in.seed = has('d') ? dummy : nullptr;
    const IpagPlan p = ipa_group_plan(opt, k < 63 ? 1ull << k : 0, protocol, np, in, hs, group, outputs, budget);
    printf("{\"err\": %d, \"msg\": ", p.err);
    if (p.msg) printf("\"%s\"", p.msg); else printf("null");           // (the plan's texts hold no quote or backslash)
    if (!p.err) {
      const IpapPlan &q = p.packed;
      const IpabPlan &b = q.base;
      printf(", \"group\": %u, \"ngroups\": %u, \"per\": %u, \"W\": %u, \"pairs\": %llu, \"route\": %u, \"rows\": %u, \"packed_total\": %llu", p.group, p.ngroups, p.per, p.W,
             (unsigned long long)p.pairs, p.route, q.rows, (unsigned long long)q.total_bytes);
      const char *names[26] = {"sa", "sb", "rec", "tab", "part", "expt", "exsc", "scale", "ab", "xs", "lr", "tr", "troff", "start", "u", "P", "c", "head", "w", "roles", "status", "T",
                               "gsa", "gsb", "E", "vals"};
      const uint64_t offs[26] = {b.o_sa, b.o_sb, b.o_rec, b.o_tab, b.o_part, b.o_expt, b.o_exsc, b.o_scale, q.o_ab, q.o_xs, q.o_lr, q.o_tr, q.o_troff, q.o_start, q.o_u, q.o_P,
                                 q.o_c, q.o_head, q.o_w, q.o_roles, q.o_status, q.o_T, p.o_gsa, p.o_gsb, p.o_E, p.o_vals};
      const uint64_t lens[26] = {b.b_sa, b.b_sb, b.b_rec, b.b_tab, b.b_part, b.b_expt, b.b_exsc, b.b_scale, q.b_ab, q.b_xs, q.b_lr, q.b_tr, q.b_troff, q.b_start, q.b_u, q.b_P,
                                 q.b_c, q.b_head, q.b_w, q.b_roles, q.b_status, q.b_T, p.b_gsa, p.b_gsb, p.b_E, p.b_vals};
      printf(", \"regions\": {");
      for (int i = 0; i < 26; i++) printf("%s\"%s\": [%llu, %llu]", i ? ", " : "", names[i], (unsigned long long)offs[i], (unsigned long long)lens[i]);
      printf("}, \"total_bytes\": %llu", (unsigned long long)p.total_bytes);
    }
    printf("}\n");
  }
  return 0;
}
