// xw_switches.hip -- the one value behind include/xnwan_switches.h: the library's switches, host-only, process-wide.  The launch
// wrappers read it through xw_switches() (xw_common.h) at each call; nothing in the library reads the environment.
#include "xw_common.h"

namespace {
XwSwitches switches = {1, 1, 1, 1, 0, 1024};
bool is_flag(int v) { return v == 0 || v == 1; }
}  // namespace

const XwSwitches& xw_switches() { return switches; }

extern "C" int xw_switches_set(const XwSwitches* s) {
  if (!s || !is_flag(s->disc_dynamic) || !is_flag(s->disc_vin_lds) || !is_flag(s->disc_rec_tsum) || !is_flag(s->duo_spread)) return XW_E_ARG;
  if (s->reduce_blocks < 0 || s->reduce_blocks > 1024) return XW_E_ARG;
  if (s->reduce_threads != 256 && s->reduce_threads != 512 && s->reduce_threads != 1024) return XW_E_ARG;
  switches = *s;
  return 0;
}

extern "C" int xw_switches_get(XwSwitches* s) {
  if (!s) return XW_E_ARG;
  *s = switches;
  return 0;
}
