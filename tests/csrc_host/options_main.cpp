// The option table of python-bulletproofs_amd/csrc/options_host.hpp printed as JSON: tests/test_options_cpu.py compiles this with the
// host compiler (address and undefined-behaviour sanitizers on) and checks the lines.
//   line 1: {"rows": [{"name", "default", "default_ok", "wide"} ...]}   default: read through the row's member from a default BpmiOptions
//   then one line per (name, value) pair of the arguments: option_set on a FRESH BpmiOptions --
//     {"rc", "msg", "fx", "stored", "rest_same"}   stored: the member read back (0 without a row); rest_same: no other member moved
#include <stdio.h>
#include <stdlib.h>

#include "options_host.hpp"

static const char *const FX[] = {"none", "graphs", "graphs_if_zero", "fold_keys"};

int main(int argc, char **argv) {
  const BpmiOptions defaults;
  printf("{\"rows\": [");
  for (int i = 0; i < OPTION_NROWS; i++) {
    const OptionRow &r = option_rows::ROWS[i];
    printf("%s{\"name\": \"%s\", \"default\": %lld, \"default_ok\": %d, \"wide\": %d}", i ? ", " : "", r.name, (long long)r.get(defaults), r.ok(r.get(defaults)) ? 1 : 0,
           r.i64 ? 1 : 0);
  }
  printf("]}\n");
  for (int a = 1; a + 1 < argc; a += 2) {
    const char *name = argv[a];
    const long long value = strtoll(argv[a + 1], nullptr, 10);
    BpmiOptions o;
    const OptionSet s = option_set(o, name, value);
    const OptionRow *mine = option_find(name);
    bool rest_same = true;
    for (const OptionRow &r : option_rows::ROWS) if (&r != mine && r.get(o) != r.get(defaults)) rest_same = false;
    if (mine && s.rc && mine->get(o) != mine->get(defaults)) rest_same = false;          // a refused value stores nothing
    printf("{\"rc\": %d, \"msg\": \"%s\", \"fx\": \"%s\", \"stored\": %lld, \"rest_same\": %d}\n", s.rc, s.msg.c_str(), FX[s.fx], mine ? (long long)mine->get(o) : 0ll,
           rest_same ? 1 : 0);
  }
  return 0;
}
