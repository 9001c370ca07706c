// How the host tests address an option: by the row of its bpmi_set_option name in the table of csrc/options_host.hpp --
// option_row("chunk") in C++, t_option_row (host_shim.cpp) from Python.  For tests only.
#pragma once
#include <stdint.h>

#include "options_host.hpp"

static inline int32_t option_row(const char *name) {       // -1: no such option
  const OptionRow *r = option_find(name);
  return r ? (int32_t)(r - option_rows::ROWS) : -1;
}
// kv: (row, value) pairs, the value stored as it is; anything not listed keeps the default of BpmiOptions
static inline BpmiOptions plan_options(const int32_t *kv, int nkv) {
  BpmiOptions o;
  for (int i = 0; i < nkv; i++) if (kv[2 * i] >= 0 && kv[2 * i] < OPTION_NROWS) option_rows::ROWS[kv[2 * i]].put(o, kv[2 * i + 1]);
  return o;
}
