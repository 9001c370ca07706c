// ipa_wire_plan_main.cpp -- the plan of a batch of BPIP2 inner-product proofs (python-bulletproofs_amd/csrc/ipa_wire_plan_host.hpp)
// printed as JSON, one line per case: tests/test_ipa_wire_plan_cpu.py compiles this with the host compiler and checks the lines.
//   ipa_wire_plan_main <k> <protocol> <n_proofs> <prefix_len> <verify> <has_scale> <t_budget> <present> <offsets> [...]
// present: one letter per array that is NOT NULL, among b(lobs) o(ff) u p(P) w(eights) d (seed); offsets: "up" (every blob 78 + 98 k +
// prefix_len bytes), "first" (off[0] = 1000, then as up), "down" (off[1] < off[0]), "short" (every blob one byte short of its fixed
// part), "huge" (two blobs, the second 2^32 bytes).  The blobs are never read by the plan: a dummy non-NULL address.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ipa_wire_plan_host.hpp"

int main(int argc, char **argv) {
  if (argc < 10 || (argc - 1) % 9) { fprintf(stderr, "usage: %s k protocol n_proofs prefix_len verify has_scale t_budget present offsets ...\n", argv[0]); return 2; }
  const BpmiOptions opt;
  static const uint8_t dummy[8] = {0};
  for (int a = 1; a + 8 < argc; a += 9) {
    const unsigned k = (unsigned)strtoul(argv[a], nullptr, 10);
    const int protocol = atoi(argv[a + 1]);
    const unsigned long long np = strtoull(argv[a + 2], nullptr, 10), prefix = strtoull(argv[a + 3], nullptr, 10);
    const int verify = atoi(argv[a + 4]), hs = atoi(argv[a + 5]);
    const unsigned long long budget = strtoull(argv[a + 6], nullptr, 10);
    const char *present = argv[a + 7], *mode = argv[a + 8];
    auto has = [&](char ch) { return strchr(present, ch) != nullptr; };
    std::vector<uint64_t> off(1);
    if (np <= IPAB_PROOFS_MAX) {
      off.resize(np + 1);
      const uint64_t first = strcmp(mode, "first") == 0 ? 1000 : 0;
      const uint64_t len = ipaw_wire_bytes(k, prefix) - (strcmp(mode, "short") == 0 ? prefix + 1 : 0);
      for (uint64_t i = 0; i <= np; i++) off[i] = first + i * len;
      if (strcmp(mode, "down") == 0 && np >= 1) { off[0] = 5; off[1] = 4; }
      if (strcmp(mode, "huge") == 0 && np >= 2) off[np] = off[np - 1] + (1ull << 32);
    }
    IpaWireIn in;
    in.blobs = has('b') ? dummy : nullptr; in.off = has('o') ? off.data() : nullptr;
    in.u = has('u') ? dummy : nullptr; in.P = has('p') ? dummy : nullptr; in.weights = has('w') ? dummy : nullptr; in.seed = has('d') ? dummy : nullptr;
    const IpawPlan p = ipa_wire_plan(opt, k, protocol, np, in, verify != 0, hs, budget);
    printf("{\"err\": %d, \"msg\": ", p.err);
    if (p.msg) printf("\"%s\"", p.msg); else printf("null");           // (the plan's texts hold no quote or backslash)
    if (!p.err) {
      const IpabPlan &b = p.base;
      printf(", \"pairs\": %u, \"wire_bytes\": %llu, \"text_bound\": %llu, \"longest\": %u, \"W\": %u, \"rows\": %u, \"base_total\": %llu", p.pairs,
             (unsigned long long)p.wire_bytes, (unsigned long long)p.text_bound, p.longest, p.W, p.rows, (unsigned long long)b.total_bytes);
      const char *names[15] = {"wire", "off", "ab", "xs", "lr", "tr", "troff", "start", "u", "P", "w", "roles", "lens", "flags", "status"};
      const uint64_t offs[15] = {p.o_wire, p.o_off, p.o_ab, p.o_xs, p.o_lr, p.o_tr, p.o_troff, p.o_start, p.o_u, p.o_P, p.o_w, p.o_roles, p.o_lens, p.o_flags, p.o_status};
      const uint64_t lens[15] = {p.b_wire, p.b_off, p.b_ab, p.b_xs, p.b_lr, p.b_tr, p.b_troff, p.b_start, p.b_u, p.b_P, p.b_w, p.b_roles, p.b_lens, p.b_flags, p.b_status};
      printf(", \"regions\": {");
      for (int i = 0; i < 15; i++) printf("\"%s\": [%llu, %llu], ", names[i], (unsigned long long)offs[i], (unsigned long long)lens[i]);
      printf("\"T\": [%llu, %llu]}, \"c_head\": [%llu, %llu], \"total_bytes\": %llu", (unsigned long long)p.o_T, (unsigned long long)p.b_T,
             (unsigned long long)p.b_c, (unsigned long long)p.b_head, (unsigned long long)p.total_bytes);
    }
    printf("}\n");
  }
  return 0;
}
