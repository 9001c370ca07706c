// ipa_packed_plan_main.cpp -- the plan of a batch of packed inner-product proofs (python-bulletproofs_amd/csrc/ipa_packed_plan_host.hpp)
// printed as JSON, one line per case: tests/test_ipa_packed_plan_cpu.py compiles this with the host compiler and checks the lines.
//   ipa_packed_plan_main <k> <protocol> <n_proofs> <tr_len> <has_scale> <present> <offsets> [...]
// present: one letter per array that is NOT NULL, among a(b) x(s) l(LR) t(ranscripts) o(tr_off) s(tart) u p(P) c h(ead) w(eights) d (seed);
// offsets: "up" (every transcript tr_len bytes), "first" (tr_off[0] = 1000, then as up), "down" (tr_off[1] < tr_off[0]).  The arrays
// other than tr_off are never read by the plan: they are dummy non-NULL addresses.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ipa_packed_plan_host.hpp"

int main(int argc, char **argv) {
  if (argc < 8 || (argc - 1) % 7) { fprintf(stderr, "usage: %s k protocol n_proofs tr_len has_scale present offsets ...\n", argv[0]); return 2; }
  const BpmiOptions opt;
  static const uint8_t dummy[8] = {0};
  for (int a = 1; a + 6 < argc; a += 7) {
    const unsigned k = (unsigned)strtoul(argv[a], nullptr, 10);
    const int protocol = atoi(argv[a + 1]);
    const unsigned long long np = strtoull(argv[a + 2], nullptr, 10), tr_len = strtoull(argv[a + 3], nullptr, 10);
    const int hs = atoi(argv[a + 4]);
    const char *present = argv[a + 5], *mode = argv[a + 6];
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
    const IpapPlan p = ipa_packed_plan(opt, k, protocol, np, in, hs);
    printf("{\"err\": %d, \"msg\": ", p.err);
    if (p.msg) printf("\"%s\"", p.msg); else printf("null");           // (the plan's texts hold no quote or backslash)
    if (!p.err) {
      const IpabPlan &b = p.base;
      printf(", \"pairs\": %u, \"n_extra\": %llu, \"rec_words\": %u, \"tr_bytes\": %llu, \"longest\": %u, \"W\": %u, \"rows\": %u, \"base_total\": %llu", p.pairs,
             (unsigned long long)b.n_extra, b.rec_words, (unsigned long long)p.tr_bytes, p.longest, p.W, p.rows, (unsigned long long)b.total_bytes);
      const char *names[22] = {"sa", "sb", "rec", "tab", "part", "expt", "exsc", "scale", "ab", "xs", "lr", "tr", "troff", "start", "u", "P", "c", "head", "w", "roles", "status", "T"};
      const uint64_t offs[22] = {b.o_sa, b.o_sb, b.o_rec, b.o_tab, b.o_part, b.o_expt, b.o_exsc, b.o_scale, p.o_ab, p.o_xs, p.o_lr, p.o_tr, p.o_troff, p.o_start, p.o_u, p.o_P,
                                 p.o_c, p.o_head, p.o_w, p.o_roles, p.o_status, p.o_T};
      const uint64_t lens[22] = {b.b_sa, b.b_sb, b.b_rec, b.b_tab, b.b_part, b.b_expt, b.b_exsc, b.b_scale, p.b_ab, p.b_xs, p.b_lr, p.b_tr, p.b_troff, p.b_start, p.b_u, p.b_P,
                                 p.b_c, p.b_head, p.b_w, p.b_roles, p.b_status, p.b_T};
      printf(", \"regions\": {");
      for (int i = 0; i < 22; i++) printf("%s\"%s\": [%llu, %llu]", i ? ", " : "", names[i], (unsigned long long)offs[i], (unsigned long long)lens[i]);
      printf("}, \"total_bytes\": %llu", (unsigned long long)p.total_bytes);
    }
    printf("}\n");
  }
  return 0;
}
