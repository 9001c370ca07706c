// msm_runs_plan_main.cpp -- the plan of the accumulation by runs (MsmGeom.runs, msm_runs_cap and the run table's shape:
// python-bulletproofs_amd/csrc/msm_plan_host.hpp) printed as JSON, one line per shape: tests/test_msm_runs_plan_cpu.py compiles this with
// the host compiler and checks the lines.
//   msm_runs_plan_main <accum_runs> <accum_runs_cap> <window_bits> <glv> <mode_bits> <n> <w0> <wcount> [...]
#include <stdio.h>
#include <stdlib.h>

#include "msm_plan_host.hpp"

int main(int argc, char **argv) {
  if (argc < 9 || (argc - 1) % 8) { fprintf(stderr, "usage: %s accum_runs accum_runs_cap window_bits glv mode_bits n w0 wcount ...\n", argv[0]); return 2; }
  for (int a = 1; a + 7 < argc; a += 8) {
    BpmiOptions opt;
    const BpmiOptions defaults;
    opt.opt_accum_runs = atoi(argv[a]);
    opt.opt_accum_runs_cap = atoi(argv[a + 1]);
    opt.opt_c = atoi(argv[a + 2]);
    opt.opt_glv = atoi(argv[a + 3]);
    const unsigned mode_bits = (unsigned)strtoul(argv[a + 4], nullptr, 10);
    MsmMode mode;
    mode.chained = mode_bits & 1u; mode.free_run = mode_bits & 2u; mode.beside = mode_bits & 4u;
    const uint64_t n = strtoull(argv[a + 5], nullptr, 10);
    const u32 w0 = (u32)strtoul(argv[a + 6], nullptr, 10), wcount = (u32)strtoul(argv[a + 7], nullptr, 10);
    const MsmPlan pl = msm_pick_geometry(opt, mode, n, w0, wcount);
    const MsmGeom &g = pl.g;
    MsmWs w;
    char *const base = (char *)(uintptr_t)(1ull << 40);       // never dereferenced: only the offsets are read back
    msm_layout(g, w, base, pl.glv);
    const u32 cap = msm_runs_cap(opt, g), bins = msm_runs_bins(cap), blocks = msm_runs_blocks(g);
    printf("{\"runs\": %u, \"cap\": %u, \"bins\": %u, \"blocks\": %u, \"n\": %u, \"c\": %u, \"W\": %u, \"G\": %u, \"top2\": %u, \"P\": %u, \"mid\": %d, \"small\": %d, \"glv\": %d, "
           "\"default_runs\": %d, \"default_cap\": %d, \"run_bins\": %u, \"run_slice\": %u, "
           "\"order_off\": %llu, \"cursor_off\": %llu, \"counts_off\": %llu, \"hist_off\": %llu, \"off_off\": %llu, \"flags_off\": %llu, \"coarse_hist_off\": %llu, "
           "\"flag_word\": %u, \"count_word\": %u, \"coarse_hist_words\": %u}\n",
           g.runs, cap, bins, blocks, g.n, g.c, g.W, g.G, g.top2, w.P, (int)pl.mid, (int)pl.small, (int)pl.glv, defaults.opt_accum_runs, defaults.opt_accum_runs_cap,
           RUN_BINS, RUN_SLICE, (unsigned long long)((char *)w.run_order - base), (unsigned long long)((char *)w.cursor - base),
           (unsigned long long)((char *)w.run_counts - base), (unsigned long long)((char *)w.hist - base), (unsigned long long)((char *)w.off - base),
           (unsigned long long)((char *)w.run_flags - base), (unsigned long long)((char *)w.coarse_hist - base), (unsigned)RUN_FLAG_WORD, (unsigned)RUN_COUNT_WORD,
           (unsigned)COARSE_HIST_WORDS);
  }
  return 0;
}
