// ipa_packed_mixed_host_main.cpp -- the host twin of the preparation of packed inner-product proofs of different lengths
// (ipap::prepare_all_mixed, python-bulletproofs_amd/csrc/ipa_packed_host.hpp, laid out by ipa_packed_mixed_plan_host.hpp the way
// bpmi_ipa_batch_prepare_mixed lays it out) as a stand-alone program: tests/test_ipa_packed_mixed_host_cpu.py builds it with the host
// compiler and the address and undefined-behaviour sanitizers.  Every input array lives in a heap block of exactly its size.
// Input (standard input, whitespace separated; arrays as hex, "-" for NULL, "." for an empty non-NULL array):
//   <cases>  then per case:  <K> <protocol> <n_classes> <threads>  weights seed   then per class:  <k> <n_proofs>  ab xs LR transcripts
//   tr_off start u P c head      (tr_off: n_proofs + 1 little-endian uint64; start: n_proofs little-endian uint32)
// Output: one JSON line per case: {"err": "..."} for an argument error, else {"rec": hex, "rec_off": [...], "pts": hex, "sc": hex,
// "status": hex}.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "ipa_packed_host.hpp"
#include "ipa_packed_mixed_plan_host.hpp"

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
    unsigned K, n_classes, threads;
    int protocol;
    if (scanf("%u %d %u %u", &K, &protocol, &n_classes, &threads) != 4 || n_classes > 64) return 2;
    Arr weights, seed;
    if (!read_arr(weights) || !read_arr(seed)) return 2;
    std::vector<Arr> arrs(10 * (size_t)n_classes);
    std::vector<bpmi_ipa_packed_class> cls(n_classes ? n_classes : 1);
    std::vector<std::vector<uint64_t>> off(n_classes);
    std::vector<std::vector<uint32_t>> start(n_classes);
    memset(cls.data(), 0, sizeof(bpmi_ipa_packed_class) * cls.size());
    for (unsigned c = 0; c < n_classes; c++) {
      unsigned k;
      unsigned long long np;
      if (scanf("%u %llu", &k, &np) != 2) return 2;
      Arr *a = &arrs[10 * (size_t)c];
      for (int i = 0; i < 10; i++) if (!read_arr(a[i])) return 2;
      // the offsets and starts go through aligned copies of their own
      off[c].resize(a[4].n / 8);
      start[c].resize(a[5].n / 4);
      if (a[4].n) memcpy(off[c].data(), a[4].p, a[4].n);
      if (a[5].n) memcpy(start[c].data(), a[5].p, a[5].n);
      if (!a[4].null && np && off[c].size() != (size_t)np + 1) return 2;
      bpmi_ipa_packed_class &q = cls[c];
      q.k = k; q.n_proofs = np;
      q.ab = a[0].p; q.xs = a[1].p; q.LR = a[2].p; q.transcripts = a[3].p;
      q.tr_off = a[4].null ? nullptr : off[c].data();
      q.start = a[5].null ? nullptr : start[c].data();
      q.u = a[6].p; q.P = a[7].p; q.c = a[8].p; q.head = a[9].p;
    }
    const IpapmPlan mp = ipa_packed_mixed_plan(BpmiOptions(), K, protocol, n_classes, cls.data(), weights.p, seed.p, 0, IPAP_T_BYTES_MAX);
    if (mp.err) {
      printf("{\"err\": \"%s\"}\n", mp.msg.c_str());
    } else {
      const size_t total = mp.empty ? 0 : (size_t)mp.base.n_proofs, pairs = mp.empty ? 0 : (size_t)mp.base.n_extra;
      std::vector<uint8_t> rec(mp.empty ? 0 : 4 * (size_t)mp.base.rec_words), pts(64 * pairs), sc(32 * pairs), status(total);
      std::vector<ipap::MixedClass> mc;
      for (u32 c : mp.fin_cls) {
        const IpapmClass &m = mp.cls[c];
        ipap::MixedClass x;
        x.k = m.k; x.n_proofs = m.n_proofs; x.gbase = m.gbase;
        x.in = ipapm_class_in(cls[c], weights.p ? weights.p + 32ull * ipap_weights(protocol) * m.gbase : nullptr, seed.p);
        x.rec = rec.data() + 4ull * m.rec_off; x.pts = pts.data() + 64 * m.extra_off; x.sc = sc.data() + 32 * m.extra_off;
        mc.push_back(x);
      }
      if (!mp.empty) ipap::prepare_all_mixed(protocol, mc, (int)threads, status.data());
      printf("{");
      print_hex("rec", rec, false);
      printf("\"rec_off\": [");
      for (unsigned c = 0; c < n_classes; c++) printf("%s%llu", c ? ", " : "", (unsigned long long)(mp.empty || !mp.cls[c].n_proofs ? 0 : 4ull * mp.cls[c].rec_off));
      printf("], ");
      print_hex("pts", pts, false);
      print_hex("sc", sc, false);
      print_hex("status", status, true);
      printf("}\n");
    }
    for (Arr &a : arrs) free(a.p);
    free(weights.p); free(seed.p);
  }
  return 0;
}
