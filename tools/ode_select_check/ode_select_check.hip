// ode_select_check.hip -- the fused stepper's kernel selection, parent's ladders against the tables: a stand-alone host program
// (hipcc --cuda-host-only -fsanitize=address,undefined; no GPU, no Python).  Both sides are compiled into ONE translation unit, so a
// kernel is the same host stub on both sides and "the same kernel, template and all parameters" is pointer equality.  The launch is
// a recorder; the CU count is the environment's FAKE_NCU (default 8); XW_DUO_SPREAD is frozen per process on the parent's side, and main sets
// the library's duo_spread switch (xw_switches.hip, linked in) from the same variable, so the program is run once per value.
//   configurations: -DXW_ODE_H=20 -DXW_ODE_K=10 | -DXW_ODE_H=64 -DXW_ODE_K=16 -DXW_ODE_WIDE16 | ... -DXW_ODE_WIDE16 -DXW_ODE_PART_RECOMP
#include <cstdio>
#include <cstring>
#include <set>
#include "xw_common.h"
#include "xnwan.h"

// a host-only build has no device code to register: the module constructor's calls end here, not in the HIP runtime
extern "C" void** __hipRegisterFatBinary(const void*) { static void* h; return &h; }
extern "C" void __hipUnregisterFatBinary(void**) {}
extern "C" void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
extern "C" void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}

static int g_ncu = 8;
struct Shot {
  const void* k;
  unsigned gx, gy, gz, bx, by, bz;
  int spread;        // BwdJobs.spread as handed to the kernel (-1: a forward launch)
  int recomp;        // 1: handed on to the recomputing object, with (method, m, params, adj) below and the job table's spread
  int method, m, params, adj, tiles, pad;
  bool operator==(const Shot& o) const { return memcmp(this, &o, sizeof(Shot)) == 0; }
};
static Shot g_rec;
static int g_launches;
static std::set<const void*> g_seen;
static_assert(sizeof(Shot) == 64, "no padding: records are compared bytewise");
static void put(const void* k, dim3 g, dim3 b, int spread) {
  memset(&g_rec, 0, sizeof(Shot));
  g_rec.k = k; g_rec.gx = g.x; g_rec.gy = g.y; g_rec.gz = g.z; g_rec.bx = b.x; g_rec.by = b.y; g_rec.bz = b.z; g_rec.spread = spread;
  ++g_launches;
  g_seen.insert(k);
}
template <class J> static int job_spread(const J& j, decltype(J::spread)*) { return j.spread; }    // BwdJobs
template <class J> static int job_spread(const J&, ...) { return -1; }                               // FwdJobs
template <class J> static void record(const void* k, dim3 g, dim3 b, const J& j) { put(k, g, b, job_spread(j, nullptr)); }

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(K, G, B, SH, ST, JOBS, ...) record((const void*)(K), dim3(G), dim3(B), JOBS)
#define xw_launch_status() 0
#define hipGetDevice(p) (*(p) = 0, hipSuccess)
#define hipDeviceGetAttribute(p, a, d) (*(p) = g_ncu, hipSuccess)

#include "xw_ode_fwd.h"      // (the recompute configuration does not include it itself; the ladders name its kernels)
#include "xw_ode.hip"
#if !defined(XW_ODE_WIDE16) && defined(XW_ODE_PART_RECOMP)
#error "the recompute configuration is built in the wide form (the parent's ladders name the narrow-tile kernels)"
#endif

#ifndef XW_ODE_PART_RECOMP
// the recomputing object of this width, as both sides call it
extern "C" int XW_ODE_FN(xw_ode_bwd_recomp_w)(const void* jobs_, const double*, const double*, int method, int, int, int m, int params,
                                              int adj, void*) {
  const BwdJobs& j = *static_cast<const BwdJobs*>(jobs_);
  memset(&g_rec, 0, sizeof(Shot));
  g_rec.recomp = 1; g_rec.method = method; g_rec.m = m; g_rec.params = params; g_rec.adj = adj; g_rec.spread = j.spread;
  g_rec.tiles = j.tile0[j.n];
  ++g_launches;
  return 0;
}
#endif

#include "old_ladders.inc"

static double buf[64];
static long n_cases, n_bad, n_kernel, n_spacer, n_recomp, n_error;
static void compare(const char* what, int rc_old, const Shot& a, int launches_old, int rc_new, const Shot& b, int launches_new, int m,
                    int method, int mode, int njobs, int pat, int tiles) {
  ++n_cases;
  n_kernel += a.k != nullptr; n_spacer += a.spread > 0; n_recomp += a.recomp; n_error += rc_old != 0;   // (what the parent did)
  if (rc_old == rc_new && launches_old == launches_new && a == b) return;
  if (++n_bad <= 20)
    printf("DISAGREE %s m=%d method=%d mode=%d njobs=%d stores=%d tiles=%d: old rc=%d k=%p grid=%u block=%u spread=%d recomp=%d | new rc=%d "
           "k=%p grid=%u block=%u spread=%d recomp=%d\n", what, m, method, mode, njobs, pat, tiles, rc_old, a.k, a.gx, a.bx, a.spread,
           a.recomp, rc_new, b.k, b.gx, b.bx, b.spread, b.recomp);
}

template <class T> static long slots(const T& table, const char* name) {
  long n = 0, missed = 0;
  for (const auto& row : table)
    for (const auto k : row.k)
      if (k) {
        ++n;
        if (!g_seen.count((const void*)k)) ++missed;
      }
  printf("  table %-14s %4ld slots, %ld never reached\n", name, n, missed);
  return missed;
}

int main() {
  const char* e = getenv("FAKE_NCU");
  if (e) g_ncu = atoi(e);
  const char* sp = getenv("XW_DUO_SPREAD");
  XwSwitches sw;
  xw_switches_get(&sw);
  sw.duo_spread = (sp ? atoi(sp) : 1) != 0;      // (as the parent's ladders read it)
  if (xw_switches_set(&sw) != 0) return 2;
  const int ncu = g_ncu > 0 ? g_ncu : 8;
  const int tile_counts[] = {ncu - 1, ncu, ncu + 1, 2 * ncu - 1, 2 * ncu, 2 * ncu + 1};
  long missed = 0;
#ifndef XW_ODE_PART_RECOMP
  // ---- forward
  for (int m = 0; m <= 11; ++m)
    for (int method = -1; method <= 3; ++method)
      for (int njobs = 1; njobs <= 4; ++njobs)
        for (int pat = 0; pat < (1 << njobs); ++pat)   // stores: bit i = job i brings one (none, all and every mixed pattern)
          for (int xo = 0; xo < 2; ++xo)
            for (int nar = 0; nar < 2; ++nar)
              for (int tiles : tile_counts) {
                XwOdeFwdJob jobs[4];
                memset(jobs, 0, sizeof(jobs));
                for (int i = 0; i < njobs; ++i) {
                  const bool st = ((pat >> i) & 1) != 0;
                  jobs[i] = XwOdeFwdJob{buf, buf, buf, buf, st ? buf : nullptr, i == 0 ? 16 * (tiles - (njobs - 1)) - 3 : 5, xo, nar, 0};
                }
                g_launches = 0; memset(&g_rec, 0, sizeof(Shot));
                const int ro = old_fwd_multi_w(jobs, njobs, buf, buf, method, 3, 2, m, nullptr, nullptr);
                const Shot a = g_rec; const int la = g_launches;
                g_launches = 0; memset(&g_rec, 0, sizeof(Shot));
                const int rn = XW_ODE_FN(xw_ode_fwd_multi_w)(jobs, njobs, buf, buf, method, 3, 2, m, nullptr, nullptr);
                compare("fwd", ro, a, la, rn, g_rec, g_launches, m, method, xo * 2 + nar, njobs, pat, tiles);
              }
  // ---- sweeps
  for (int m = 0; m <= 11; ++m)
    for (int method = -1; method <= 3; ++method)
      for (int mode = 0; mode <= 255; ++mode)
        for (int njobs = 1; njobs <= 4; ++njobs)
          for (int pat = 0; pat < (1 << njobs); ++pat)
            for (int tiles : tile_counts) {
              XwOdeBwdJob jobs[4];
              memset(jobs, 0, sizeof(jobs));
              for (int i = 0; i < njobs; ++i) {
                const bool st = ((pat >> i) & 1) != 0;
                jobs[i].xT = jobs[i].start = jobs[i].Y = jobs[i].ubar = buf;
                jobs[i].act = st ? buf : nullptr;
                jobs[i].gx = jobs[i].gs = jobs[i].gslab = buf;
                jobs[i].N = i == 0 ? 16 * (tiles - (njobs - 1)) - 3 : 5;
              }
              g_launches = 0; memset(&g_rec, 0, sizeof(Shot));
              const int ro = old_bwd_multi_w(jobs, njobs, buf, buf, method, 3, 2, m, mode, nullptr);
              const Shot a = g_rec; const int la = g_launches;
              g_launches = 0; memset(&g_rec, 0, sizeof(Shot));
              const int rn = XW_ODE_FN(xw_ode_bwd_multi_w)(jobs, njobs, buf, buf, method, 3, 2, m, mode, nullptr);
              compare("bwd", ro, a, la, rn, g_rec, g_launches, m, method, mode, njobs, pat, tiles);
            }
  missed += slots(fwd_table, "fwd_table");
  missed += slots(sweep_table, "sweep_table");
#else
  // ---- the recomputing object: every (m, method, params, adj) a sweep entry can hand on, and beyond
  BwdJobs J;
  memset(&J, 0, sizeof(J));
  for (int m = 0; m <= 11; ++m)
    for (int method = -1; method <= 3; ++method)
      for (int params = 0; params <= 2; ++params)
        for (int adj = 0; adj <= 2; ++adj)
          for (int tiles : tile_counts) {
            J.n = 2; J.tile0[1] = 1; J.tile0[2] = tiles;
            g_launches = 0; memset(&g_rec, 0, sizeof(Shot));
            const int ro = old_recomp_w(&J, buf, buf, method, 3, 2, m, params, adj, nullptr);
            const Shot a = g_rec; const int la = g_launches;
            g_launches = 0; memset(&g_rec, 0, sizeof(Shot));
            const int rn = XW_ODE_FN(xw_ode_bwd_recomp_w)(&J, buf, buf, method, 3, 2, m, params, adj, nullptr);
            compare("recomp", ro, a, la, rn, g_rec, g_launches, m, method, params * 2 + adj, 2, 0, tiles);
          }
  missed += slots(recomp_table, "recomp_table");
#endif
  printf("H=%d K=%d ncu=%d XW_DUO_SPREAD=%s: %ld cases (%ld kernel launches, %ld of them with a spacer round, %ld handed to the recomputing "
         "object, %ld errors), %ld disagreements, %ld table slots never reached\n", XW_ODE_H, XW_ODE_K, g_ncu, sp ? sp : "(unset)", n_cases,
         n_kernel, n_spacer, n_recomp, n_error, n_bad, missed);
  return n_bad || missed ? 1 : 0;
}
