// ipa_prove_mixed_plan_main.cpp -- the plan of the batched inner-product prover's mixed calls
// (python-bulletproofs_amd/csrc/ipa_prove_mixed_plan_host.hpp) printed as JSON: tests/test_ipa_prove_mixed_plan_cpu.py compiles this with
// the host compiler and checks the lines.
//   ipa_prove_mixed_plan_main bases                          the lists of every class of the capacities 1, 2, 8, 1 024; ipp_class_bases(n, n) against ipp_plan
//   ipa_prove_mixed_plan_main args N n:count ...             ippm_args_error of the classes
//   ipa_prove_mixed_plan_main many N classes n count         ippm_args_error of `classes` equal classes
//   ipa_prove_mixed_plan_main plan N protocol job_lanes n:count:seed_max:have_c ...
//   ipa_prove_mixed_plan_main commit N u_mode job_lanes n:count:have_a:have_b:have_t ...
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ipa_prove_mixed_plan_host.hpp"

static void print_list(const std::vector<unsigned short> &v) {
  printf("[");
  for (size_t i = 0; i < v.size(); i++) printf(i ? ",%u" : "%u", (unsigned)v[i]);
  printf("]");
}
static std::vector<unsigned long long> fields(const char *s) {
  std::vector<unsigned long long> out;
  for (const char *p = s; *p;) {
    char *end = nullptr;
    out.push_back(strtoull(p, &end, 10));
    p = *end ? end + 1 : end;
  }
  return out;
}
static void print_units(const std::vector<RppmUnit> &units, const std::vector<IppmLaunch> &launches) {
  printf("\"launches\": [");
  for (size_t i = 0; i < launches.size(); i++) {
    const IppmLaunch &L = launches[i];
    printf("%s{\"kind\": \"%s\", \"step\": %u, \"threads\": %u, \"gl\": %u, \"round\": %u, \"first\": %u, \"blocks\": %u, \"units\": [", i ? ", " : "", ippm_kind_name(L.kind), L.step,
           L.threads, L.gl, L.round, L.first, L.blocks);
    for (u32 u = 0; u < L.n_units; u++) printf("%s[%u, %u]", u ? ", " : "", units[L.first_unit + u].cls, units[L.first_unit + u].first);
    printf("]}");
  }
  printf("], \"n_units\": %zu", units.size());
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  if (mode == "bases") {
    printf("{\"own\": {");
    for (u32 n = 1; n <= 1024; n <<= 1) printf("%s\"%u\": %s", n > 1 ? ", " : "", n, ipp_class_bases(n, n) == ipp_plan(n, 0).bases && ipp_class_bases_len(n) == ipp_plan(n, 0).bases.size() ? "true" : "false");
    printf("}, \"capacities\": {");
    const u32 Ns[] = {1, 2, 8, 1024};
    for (int i = 0; i < 4; i++) {
      const u32 N = Ns[i];
      const std::vector<unsigned short> all = ipp_capacity_bases(N), call = ipp_capacity_commit_bases(N);
      printf("%s\"%u\": {\"total\": %zu, \"commit_total\": %zu, \"end\": %zu, \"commit_end\": %zu, \"classes\": {", i ? ", " : "", N, all.size(), call.size(), ipp_capacity_bases_off(N, 2 * N),
             ipp_capacity_commit_bases_off(N, 2 * N));
      for (u32 n = 1; n <= N; n <<= 1) {
        const size_t off = ipp_capacity_bases_off(N, n), coff = ipp_capacity_commit_bases_off(N, n);
        printf("%s\"%u\": {\"off\": %zu, \"len\": %zu, \"commit_off\": %zu, \"bases\": ", n > 1 ? ", " : "", n, off, ipp_class_bases_len(n), coff);
        print_list(std::vector<unsigned short>(all.begin() + off, all.begin() + off + ipp_class_bases_len(n)));
        printf(", \"commit_bases\": ");
        print_list(std::vector<unsigned short>(call.begin() + coff, call.begin() + coff + 4 * n + 3));
        printf(", \"commit_offsets\": [%u, %u, %u]}", ipp_commit_bases_offset(n, true, true), ipp_commit_bases_offset(n, true, false), ipp_commit_bases_offset(n, false, true));
      }
      printf("}}");
    }
    printf("}}\n");
    return 0;
  }
  if (mode == "args" || mode == "many") {
    const u32 N = (u32)strtoul(argv[2], nullptr, 10);
    std::vector<IppmClassIn> in;
    u32 n_classes = 0;
    if (mode == "many") {
      n_classes = (u32)strtoul(argv[3], nullptr, 10);
      IppmClassIn k; k.n = (u32)strtoul(argv[4], nullptr, 10); k.count = strtoull(argv[5], nullptr, 10);
      in.assign(n_classes, k);
    } else {
      for (int a = 3; a < argc; a++) { const auto f = fields(argv[a]); IppmClassIn k; k.n = (u32)f[0]; k.count = f[1]; in.push_back(k); }
      n_classes = (u32)in.size();
    }
    const std::string bad = ippm_args_error(N, n_classes, in.data());
    printf("{\"msg\": \"%s\", \"null_classes\": \"%s\"}\n", bad.c_str(), ippm_args_error(N, 1, nullptr).c_str());
    return 0;
  }
  if (mode == "plan") {
    const u32 N = (u32)strtoul(argv[2], nullptr, 10);
    const int protocol = atoi(argv[3]), lanes = atoi(argv[4]);
    std::vector<IppmClassIn> in;
    for (int a = 5; a < argc; a++) { const auto f = fields(argv[a]); IppmClassIn k; k.n = (u32)f[0]; k.count = f[1]; k.seed_max = f[2]; k.have_c = f[3] != 0; in.push_back(k); }
    const IppmPlan p = ipp_mixed_plan(N, protocol, (u32)in.size(), in.data(), lanes);
    printf("{\"err\": %d, \"msg\": \"%s\"", p.err, p.msg.c_str());
    if (!p.err) {
      printf(", \"N\": %u, \"k_max\": %u, \"nsteps\": %u, \"n_proofs\": %llu, \"o_P\": %zu, \"o_P_end\": %zu, \"o_batch\": %zu, \"o_affine\": %zu, \"o_jobs\": %zu, \"o_units\": %zu, "
             "\"in_bytes\": %zu, \"o_out\": %zu, \"need\": %zu, \"slots\": [%u, %u, %u, %zu], \"classes\": [",
             p.N, p.k_max, p.nsteps, (unsigned long long)p.n_proofs, p.o_P, p.o_P_end, p.o_batch, p.o_affine, p.o_jobs, p.o_units, p.in_bytes, p.o_out, p.need, IPPM_BATCH_SLOT,
             IPPM_AFFINE_SLOT, IPPM_JOBS_SLOT, sizeof(RppmUnit));
      for (size_t c = 0; c < p.cls.size(); c++) {
        const IppmClass &q = p.cls[c];
        printf("%s{\"n\": %u, \"k\": %u, \"NT\": %u, \"per_block\": %u, \"count\": %llu, \"first\": %llu, \"bases_off\": %zu, \"tr_bytes\": %llu, \"dig0_stride\": %u, \"tr_stride\": %u, "
               "\"inputs\": {\"dig0\": %zu, \"dlen\": %zu, \"ain\": %zu, \"bin\": %zu, \"cin\": %zu, \"Pin\": %zu}, "
               "\"scratch\": {\"uc\": %zu, \"hsc\": %zu, \"xr\": %zu, \"a\": %zu, \"b\": %zu, \"cg\": %zu, \"hf\": %zu, \"jsc\": %zu, \"jout\": %zu}, "
               "\"outputs\": {\"ab\": %zu, \"xs\": %zu, \"lr\": %zu, \"head\": %zu, \"trlen\": %zu, \"tr\": %zu}}",
               c ? ", " : "", q.n, q.k, q.NT, q.per_block, (unsigned long long)q.count, (unsigned long long)q.first, q.bases_off, (unsigned long long)q.tr_bytes, q.dig0_stride,
               q.tr_stride, q.o_dig0, q.o_dlen, q.o_ain, q.o_bin, q.o_cin, q.o_Pin, q.o_uc, q.o_hsc, q.o_xr, q.o_a, q.o_b, q.o_cg, q.o_hf, q.o_jsc, q.o_jout, q.o_ab, q.o_xs, q.o_lr,
               q.o_head, q.o_trlen, q.o_tr);
      }
      printf("], ");
      print_units(p.units, p.launches);
      printf(", \"jobs\": [");
      for (size_t i = 0; i < p.jobs.size(); i++) {
        const IppmJobs &j = p.jobs[i];
        printf("%s[%u, %u, %u, %u, %u, %u]", i ? ", " : "", j.njobs, j.ntypes, j.T, j.stride, j.base_off, j.from_hsc);
      }
      printf("]");
    }
    printf("}\n");
    return 0;
  }
  if (mode == "commit") {
    const u32 N = (u32)strtoul(argv[2], nullptr, 10);
    const int u_mode = atoi(argv[3]), lanes = atoi(argv[4]);
    std::vector<IppmClassIn> in;
    for (int a = 5; a < argc; a++) {
      const auto f = fields(argv[a]);
      IppmClassIn k; k.n = (u32)f[0]; k.count = f[1]; k.have_a = f[2] != 0; k.have_b = f[3] != 0; k.have_t = f[4] != 0;
      in.push_back(k);
    }
    const IppmCommitPlan p = ipp_mixed_commit_plan(N, u_mode, (u32)in.size(), in.data(), lanes);
    printf("{\"err\": %d, \"msg\": \"%s\"", p.err, p.msg.c_str());
    if (!p.err) {
      printf(", \"count\": %llu, \"o_commit\": %zu, \"o_affine\": %zu, \"o_jobs\": %zu, \"o_units\": %zu, \"in_bytes\": %zu, \"o_out\": %zu, \"need\": %zu, \"slots\": [%u, %u, %u, %zu], \"classes\": [",
             (unsigned long long)p.count, p.o_commit, p.o_affine, p.o_jobs, p.o_units, p.in_bytes, p.o_out, p.need, IPPM_COMMIT_SLOT, IPPM_AFFINE_SLOT, IPPM_JOBS_SLOT, sizeof(RppmUnit));
      for (size_t c = 0; c < p.cls.size(); c++) {
        const IppmCommitClass &q = p.cls[c];
        printf("%s{\"n\": %u, \"NT\": %u, \"per_block\": %u, \"T\": %u, \"count\": %llu, \"bases_off\": %zu, \"ain\": %zu, \"bin\": %zu, \"tin\": %zu, \"jsc\": %zu, \"jout\": %zu, \"pts\": %zu}",
               c ? ", " : "", q.n, q.NT, q.per_block, q.T, (unsigned long long)q.count, q.bases_off, q.o_ain, q.o_bin, q.o_tin, q.o_jsc, q.o_jout, q.o_pts);
      }
      printf("], ");
      print_units(p.units, p.launches);
    }
    printf("}\n");
    return 0;
  }
  return 2;
}
