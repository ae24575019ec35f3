// check.hip -- the test network's kernel selection under the library switches: a stand-alone host program (hipcc --cuda-host-only
// -fsanitize=address,undefined; no GPU, no Python, no HIP runtime).  ONE translation unit: a host-only object with kernels refers to
// a device image of its own, which only this file's registration stand-ins take the place of.  run.sh builds and runs it.
#include "recorder.h"

// a host-only build has no device code to register: the module constructor's calls end here, not in the HIP runtime
extern "C" void** __hipRegisterFatBinary(const void*) { static void* h; return &h; }
extern "C" void __hipUnregisterFatBinary(void**) {}
extern "C" void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
extern "C" void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}

#include "check_fwd.hip"
#include "check_bwd.hip"

int main(int argc, char** argv) {
  const bool wrong = argc > 1 && !strcmp(argv[1], "--wrong");
  long bad = 0;
  XwSwitches keep;
  xw_switches_get(&keep);
  printf("| disc_vin_lds | disc_dynamic | disc_rec_tsum | forward cases | launch a kernel | generic path | reverse cases | launch a kernel | from the record | generic path | error code | distinct kernels | disagreements |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|\n");
  for (int s = 7; s >= 0; --s) {
    XwSwitches sw = keep;
    sw.disc_vin_lds = (s >> 2) & 1; sw.disc_dynamic = (s >> 1) & 1; sw.disc_rec_tsum = s & 1;
    if (xw_switches_set(&sw) != 0) return 2;
    const Tally f = check_fwd(sw, wrong), b = check_bwd(sw.disc_rec_tsum, wrong);
    printf("| %d | %d | %d | %ld | %ld | %ld | %ld | %ld | %ld | %ld | %ld | %ld | %ld |\n", sw.disc_vin_lds, sw.disc_dynamic, sw.disc_rec_tsum,
           f.cases, f.kernel, f.generic, b.cases, b.kernel, b.rec, b.generic, f.error + b.error, (long)g_kernels.size(), f.bad + b.bad);
    bad += f.bad + b.bad;
  }
  xw_switches_set(&keep);
  printf("(distinct kernels: cumulative over the settings.)  %ld disagreements%s\n", bad, wrong ? " (--wrong: the expectation took the switches inverted; there must be some)" : "");
  return wrong ? (bad ? 0 : 1) : (bad ? 1 : 0);
}
