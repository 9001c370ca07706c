// msm_fixed_plan_main.cpp -- the plan of a fixed-base MSM (python-bulletproofs_amd/csrc/msm_fixed_plan_host.hpp) printed as JSON, one line
// per shape: tests/test_msm_fixed_plan_cpu.py compiles this with the host compiler and checks the lines.
//   msm_fixed_plan_main <accum_runs> <chained> <n> <window_bits> <rows> [...]
#include <stdio.h>
#include <stdlib.h>

#include "msm_fixed_plan_host.hpp"

static void print_geom(const char *name, const MsmGeom &g) {
  printf(", \"%s\": {\"n\": %u, \"c\": %u, \"W\": %u, \"w0\": %u, \"B\": %u, \"G\": %u, \"L\": %u, \"nv\": %u, \"prio\": %u, \"fuse\": %u, \"top2\": %u, \"runs\": %u, \"inblock\": %u}",
         name, g.n, g.c, g.W, g.w0, g.B, g.G, g.L, g.nv, g.prio, g.fuse, g.top2, g.runs, g.inblock);
}

int main(int argc, char **argv) {
  if (argc < 6 || (argc - 1) % 5) { fprintf(stderr, "usage: %s accum_runs chained n window_bits rows ...\n", argv[0]); return 2; }
  for (int a = 1; a + 4 < argc; a += 5) {
    BpmiOptions opt;
    opt.opt_accum_runs = atoi(argv[a]);
    MsmMode mode;
    mode.chained = atoi(argv[a + 1]) != 0;
    const uint64_t n = strtoull(argv[a + 2], nullptr, 10);
    const u32 c = (u32)strtoul(argv[a + 3], nullptr, 10), rows = (u32)strtoul(argv[a + 4], nullptr, 10);
    const FixedPlan p = fixed_plan(n, c, rows);
    printf("{\"err\": %d, \"msg\": ", p.err);
    if (p.msg) printf("\"%s\"", p.msg); else printf("null");           // (the plan's texts hold no quote or backslash)
    if (!p.err) {
      printf(", \"n\": %llu, \"c\": %u, \"W\": %u, \"R\": %u, \"Wv\": %u, \"table_bytes\": %llu, \"pairs_max\": %llu", (unsigned long long)p.n, p.c, p.W, p.R, p.Wv,
             (unsigned long long)p.table_bytes, (unsigned long long)FIXED_PAIRS_MAX);
      if (p.c) {
        printf(", \"map\": [");
        for (u32 w = 0; w < p.W; w++) { const FixedSlot s = fixed_window_slot(w, p.Wv); printf("%s[%u, %u]", w ? ", " : "", s.wv, s.r); }
        printf("]");
        const MsmGeom real = fixed_real_geometry(p);
        print_geom("real", real);
        if (p.R > 1u) {
          const MsmPlan v = fixed_virtual_geometry(opt, mode, p);
          // the ordinary pipeline MSM of that size and width: forced window bits, a window group of Wv windows
          BpmiOptions forced = opt;
          forced.opt_c = (int)p.c;
          const MsmPlan o = msm_pick_geometry(forced, mode, p.n * p.R, 0, p.Wv);
          print_geom("virtual", v.g);
          print_geom("ordinary", o.g);
          MsmWs wv, wo;
          msm_layout(v.g, wv, nullptr, v.glv);
          msm_layout(o.g, wo, nullptr, o.glv);
          printf(", \"family\": [%d, %d, %d], \"ws\": %llu, \"ws_ordinary\": %llu, \"P\": %u, \"dig16_codes\": %llu, \"negs\": %u", v.mid ? 1 : 0, v.small ? 1 : 0, v.glv ? 1 : 0,
                 (unsigned long long)wv.total, (unsigned long long)wo.total, wv.P, (unsigned long long)v.g.n * v.g.W, v.g.n);
        }
      }
    }
    printf("}\n");
  }
  return 0;
}
