// mmadd_main.cpp -- the affine + affine addition of the accumulation by runs (xyzz_mmadd, python-bulletproofs_amd/csrc/curve.hpp) and the
// host predicate that picks the dense instantiation of k_accum_runs (segs_one_dense, shared_defs.hpp), driven from stdin, one case per line:
//   mmadd <9 limbs x1> <9 limbs y1> <9 limbs x2> <9 limbs y2>     -> the 36 limbs X, Y, ZZ, ZZZ of xyzz_mmadd (hex); the record aliases x1 / y1
//                                                                     as the kernel's accumulator does
//   dbl <9 limbs x> <9 limbs y>                                   -> the 36 limbs of xyzz_dbl_affine
//   dense <n0> <n1> <n2> <total> <hlog0> <hlog1> <hlog2> <phase0> <phase1> <phase2> <glv>     -> 0 or 1
// Limbs are given raw (hex), so a case can sit on the edge of an operand's limb contract.  tests/test_mmadd_host_cpu.py compiles this with
// the host compiler under ASan + UBSan and checks the lines against Python integers.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "shared_defs.hpp"

using namespace bpmi;

static bool read_fe(fe &r) {
  for (int k = 0; k < 9; k++) { unsigned v; if (scanf("%x", &v) != 1) return false; r.v[k] = v; }
  return true;
}
static void print_xyzz(const xyzz &a) {
  const fe *f[4] = {&a.X, &a.Y, &a.ZZ, &a.ZZZ};
  for (int i = 0; i < 4; i++) for (int k = 0; k < 9; k++) printf("%x%c", f[i]->v[k], (i == 3 && k == 8) ? '\n' : ' ');
}

int main() {
  char op[16];
  while (scanf("%15s", op) == 1) {
    if (!strcmp(op, "mmadd")) {
      xyzz acc;
      fe x2, y2;
      if (!read_fe(acc.X) || !read_fe(acc.Y) || !read_fe(x2) || !read_fe(y2)) return 2;
      fe_set_one(acc.ZZ); fe_set_one(acc.ZZZ);
      xyzz_mmadd(acc, acc.X, acc.Y, x2, y2);
      print_xyzz(acc);
    } else if (!strcmp(op, "dbl")) {
      fe x, y;
      xyzz r;
      if (!read_fe(x) || !read_fe(y)) return 2;
      xyzz_dbl_affine(r, x, y);
      print_xyzz(r);
    } else if (!strcmp(op, "dense")) {
      unsigned v[11];
      for (int k = 0; k < 11; k++) if (scanf("%u", &v[k]) != 1) return 2;
      static const u32 pts[4] = {0, 0, 0, 0};          // never dereferenced
      Segs s = segs_init();
      for (int k = 0; k < 3; k++) { s.n[k] = v[k]; s.pts[k] = v[k] ? pts : nullptr; s.sc[k] = v[k] ? pts : nullptr; s.hlog[k] = v[4 + k]; s.phase[k] = v[7 + k]; }
      s.total = v[3];
      if (v[10]) { s.glv_sub = pts; s.glv_bx = pts; s.glv_neg = (const unsigned char *)pts; }
      printf("%d\n", segs_one_dense(s) ? 1 : 0);
    } else {
      fprintf(stderr, "unknown case '%s'\n", op);
      return 2;
    }
  }
  return 0;
}
