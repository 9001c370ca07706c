// ipa_packed_host_main.cpp -- the host twin of the packed inner-product batch preparation (python-bulletproofs_amd/csrc/
// ipa_packed_host.hpp) as a stand-alone program: tests/test_ipa_packed_host_cpu.py builds it with the host compiler and the address
// and undefined-behaviour sanitizers and compares its lines with Python integers and the oracle's verifiers.  Every input array
// lives in a heap block of exactly its size, so a read past the end of the last transcript is the sanitizer's to report.
// Input (standard input, whitespace separated; arrays as hex, "-" for NULL, "." for an empty non-NULL array):
//   <cases>  then per case:  <k> <protocol> <n_proofs> <threads>  ab xs LR transcripts tr_off start u P c head weights seed
//   (tr_off: n_proofs + 1 little-endian uint64; start: n_proofs little-endian uint32)
// Output: one JSON line per case: {"err": "..."} for an argument error, else {"rec": hex, "pts": hex, "sc": hex, "status": hex}.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "ipa_packed_host.hpp"

struct Arr { uint8_t *p = nullptr; size_t n = 0; bool null = true; };

static bool read_arr(Arr &a) {
  static std::vector<char> tok(1 << 22);
  if (scanf("%4194303s", tok.data()) != 1) return false;
  const size_t len = strlen(tok.data());
  if (len == 1 && tok[0] == '-') return true;
  a.null = false;
  if (len == 1 && tok[0] == '.') { a.p = (uint8_t *)malloc(1); return true; }          // non-NULL, nothing readable that matters
  if (len % 2) return false;
  a.n = len / 2;
  a.p = (uint8_t *)malloc(a.n);
  for (size_t i = 0; i < a.n; i++) {
    unsigned v;
    if (sscanf(tok.data() + 2 * i, "%2x", &v) != 1) return false;
    a.p[i] = (uint8_t)v;
  }
  return true;
}
static void print_hex(const char *name, const std::vector<uint8_t> &v, bool last) {
  printf("\"%s\": \"", name);
  for (uint8_t b : v) printf("%02x", b);
  printf(last ? "\"" : "\", ");
}

int main() {
  unsigned cases;
  if (scanf("%u", &cases) != 1) return 2;
  for (unsigned cs = 0; cs < cases; cs++) {
    unsigned k, proofs, threads;
    int protocol;
    if (scanf("%u %d %u %u", &k, &protocol, &proofs, &threads) != 4) return 2;
    Arr a[12];
    for (int i = 0; i < 12; i++) if (!read_arr(a[i])) return 2;
    IpaPackedIn in;
    in.ab = a[0].p; in.xs = a[1].p; in.LR = a[2].p; in.transcripts = a[3].p;
    // the offsets and starts go through aligned copies of their own
    std::vector<uint64_t> off(a[4].n / 8);
    std::vector<uint32_t> start(a[5].n / 4);
    if (a[4].n) memcpy(off.data(), a[4].p, a[4].n);
    if (a[5].n) memcpy(start.data(), a[5].p, a[5].n);
    in.tr_off = a[4].null ? nullptr : off.data();
    in.start = a[5].null ? nullptr : start.data();
    in.u = a[6].p; in.P = a[7].p; in.c = a[8].p; in.head = a[9].p; in.weights = a[10].p; in.seed = a[11].p;
    if (!a[4].null && off.size() != (size_t)proofs + 1) return 2;
    const IpapPlan pl = ipa_packed_plan(BpmiOptions(), k, protocol, proofs, in, 0);
    if (pl.err) {
      printf("{\"err\": \"%s\"}\n", pl.msg);
    } else {
      const size_t pairs = (size_t)ipap_pairs(k, protocol) * proofs;
      std::vector<uint8_t> rec((64 * (size_t)k + 96) * proofs), pts(64 * pairs), sc(32 * pairs), status(proofs);
      ipap::prepare_all(k, protocol, proofs, in, (int)threads, rec.data(), pts.data(), sc.data(), status.data());
      printf("{");
      print_hex("rec", rec, false);
      print_hex("pts", pts, false);
      print_hex("sc", sc, false);
      print_hex("status", status, true);
      printf("}\n");
    }
    for (int i = 0; i < 12; i++) free(a[i].p);
  }
  return 0;
}
