// old_ladders.inc -- the stepper's launch ladders as they stood in commit 7ef492e (xw_ode.hip: the depth switch (here OLD_ODE_DISPATCH), launch_fwd, the three entry
// points; xw_ode_mfma4.h / xw_ode_mfma16.h: launch_fwd_narrow, launch_bwd), names prefixed old_; the launch is ode_select_check.hip's recorder
#ifdef XW_ODE_ONLY_M      /* development builds (ISA listings, A/B variants): one depth only */
#define OLD_ODE_DISPATCH(CALL)                                    \
  switch (m) {                                                   \
    case XW_ODE_ONLY_M: { CALL(XW_ODE_H, XW_ODE_K, XW_ODE_ONLY_M) } \
    default: return XW_E_DIMS;                                   \
  }
#else
#define OLD_ODE_DISPATCH(CALL)                                    \
  switch (m) {                                                   \
    case 1: { CALL(XW_ODE_H, XW_ODE_K, 1) }                      \
    case 2: { CALL(XW_ODE_H, XW_ODE_K, 2) }                      \
    case 3: { CALL(XW_ODE_H, XW_ODE_K, 3) }                      \
    case 4: { CALL(XW_ODE_H, XW_ODE_K, 4) }                      \
    case 5: { CALL(XW_ODE_H, XW_ODE_K, 5) }                      \
    case 6: { CALL(XW_ODE_H, XW_ODE_K, 6) }                      \
    case 7: { CALL(XW_ODE_H, XW_ODE_K, 7) }                      \
    case 8: { CALL(XW_ODE_H, XW_ODE_K, 8) }                      \
    case 9: { CALL(XW_ODE_H, XW_ODE_K, 9) }                      \
    case 10: { CALL(XW_ODE_H, XW_ODE_K, 10) }                    \
    default: return XW_E_DIMS;                                   \
  }
#endif
namespace {
#ifdef XW_ODE_WIDE16
template <int H, int K, int M>
bool old_launch_fwd_narrow(int, const FwdJobs&, const double*, const double*, int, int, dim3, hipStream_t, int&) { return false; }
template <int H, int K, int M, bool PARAMS>
int old_launch_bwd(int method, const BwdJobs& jobs, const double* t, const double* theta, int L, int d, bool adj, bool narrow,
               hipStream_t s) {
  const dim3 grid(jobs.tile0[jobs.n]), block(64);
  // the wide container: no narrow tiles; the recomputing sweeps form their weight gradients themselves (OUTER = 1)
  bool act_ = true;
  for (int i = 0; i < jobs.n; ++i) act_ = act_ && jobs.act[i] != nullptr;
  if (adj || !act_ || method > 1)
    return XW_ODE_FN(xw_ode_bwd_recomp_w)(&jobs, t, theta, method, L, d, M, PARAMS ? 1 : 0, adj ? 1 : 0, (void*)s);
  // from the activation store: without weight gradients one wave per tile, with them the duo sweep (chain wave + partner wave)
  if (PARAMS) {
    BwdJobs jd = jobs;
    jd.spread = 0;
    if (method == 0) hipLaunchKernelGGL((k_ode_bwd_duo<H, K, M, 0>), grid, dim3(XW_DUO_THREADS), 0, s, jd, t, theta, L, d);
    else hipLaunchKernelGGL((k_ode_bwd_duo<H, K, M, 1>), grid, dim3(XW_DUO_THREADS), 0, s, jd, t, theta, L, d);
  } else {
    if (method == 0) hipLaunchKernelGGL((k_ode_bwd<H, K, M, 0, false, true>), grid, block, 0, s, jobs, t, theta, L, d);
    else hipLaunchKernelGGL((k_ode_bwd<H, K, M, 1, false, true>), grid, block, 0, s, jobs, t, theta, L, d);
  }
  return xw_launch_status();
}
#else
template <int H, int K, int M>
bool old_launch_fwd_narrow(int sel, const FwdJobs& jobs, const double* t, const double* theta, int L, int d, dim3 grid, hipStream_t s, int& rc) {
  if (!jobs.narrow) return false;
  rc = XW_E_ARG;
  switch (sel) {
    case 0: hipLaunchKernelGGL((n4::k_ode_fwd_n4<H, K, M, 0, 0>), grid, dim3(256), 0, s, jobs, t, theta, L, d); break;
    case 1: hipLaunchKernelGGL((n4::k_ode_fwd_n4<H, K, M, 0, 1>), grid, dim3(256), 0, s, jobs, t, theta, L, d); break;
    case 2: hipLaunchKernelGGL((n4::k_ode_fwd_n4<H, K, M, 0, 2>), grid, dim3(256), 0, s, jobs, t, theta, L, d); break;
    case 3: hipLaunchKernelGGL((n4::k_ode_fwd_n4<H, K, M, 1, 0>), grid, dim3(256), 0, s, jobs, t, theta, L, d); break;
    case 4: hipLaunchKernelGGL((n4::k_ode_fwd_n4<H, K, M, 1, 1>), grid, dim3(256), 0, s, jobs, t, theta, L, d); break;
    case 5: hipLaunchKernelGGL((n4::k_ode_fwd_n4<H, K, M, 1, 2>), grid, dim3(256), 0, s, jobs, t, theta, L, d); break;
    case 6: hipLaunchKernelGGL((n4::k_ode_fwd_n4<H, K, M, 2, 0>), grid, dim3(256), 0, s, jobs, t, theta, L, d); break;
    default: return true;
  }
  rc = xw_launch_status();
  return true;
}
template <int H, int K, int M, bool PARAMS>
int old_launch_bwd(int method, const BwdJobs& jobs, const double* t, const double* theta, int L, int d, bool adj, bool narrow,
               hipStream_t s) {
  const dim3 grid(jobs.tile0[jobs.n]), block(64);
  if (narrow) {
    // narrow tiles (xw_ode_n4.h): the same grid of 16-path tiles, four waves of 4 paths each; from the activation store only
    if (adj || method > 1) return XW_E_ARG;
    for (int i = 0; i < jobs.n; ++i)
      if (jobs.act[i] == nullptr) return XW_E_ARG;
    if (method == 0) hipLaunchKernelGGL((n4::k_ode_bwd_n4<H, K, M, 0, PARAMS>), grid, dim3(256), 0, s, jobs, t, theta, L, d);
    else hipLaunchKernelGGL((n4::k_ode_bwd_n4<H, K, M, 1, PARAMS>), grid, dim3(256), 0, s, jobs, t, theta, L, d);
    return xw_launch_status();
  }
  bool act = true;                                     // all jobs or none (checked by the caller)
  for (int i = 0; i < jobs.n; ++i) act = act && jobs.act[i] != nullptr;
  if (adj || !act || method > 1)      // (the recomputing sweeps live in an object of their own: xw_ode.hip, XW_ODE_PART_RECOMP)
    return XW_ODE_FN(xw_ode_bwd_recomp_w)(&jobs, t, theta, method, L, d, M, PARAMS ? 1 : 0, adj ? 1 : 0, (void*)s);
  // two rounds of tiles over the CUs: a spacer round in between (k_ode_bwd_duo)
  static const int spread_on = [] { const char* e = getenv("XW_DUO_SPREAD"); return e ? atoi(e) : 1; }();
  static const int ncu = [] { int dev = 0, n = 0; if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 0; return n; }();
  const int tiles = jobs.tile0[jobs.n];
  BwdJobs jd = jobs;
  // (exactly two rounds: 103 against 142 us at 512 tiles; with three rounds the third block of a CU meets the first again either
  //  way -- 149 against 145 us --, and from four rounds on every SIMD hosts two waves whatever the order)
  jd.spread = (spread_on && ncu > 0 && tiles > ncu && tiles <= 2 * ncu) ? ncu : 0;
  const int rounds = jd.spread ? (tiles + ncu - 1) / ncu : 0;
  const dim3 duo_grid(jd.spread ? (2 * (rounds - 1)) * ncu + (tiles - (rounds - 1) * ncu) : tiles);
  switch (method) {
    case 0:
      if (PARAMS) hipLaunchKernelGGL((k_ode_bwd_duo<H, K, M, 0>), duo_grid, dim3(XW_DUO_THREADS), 0, s, jd, t, theta, L, d);
      else hipLaunchKernelGGL((k_ode_bwd<H, K, M, 0, false, true>), grid, block, 0, s, jobs, t, theta, L, d);
      break;
    case 1:
      if (PARAMS) hipLaunchKernelGGL((k_ode_bwd_duo<H, K, M, 1>), duo_grid, dim3(XW_DUO_THREADS), 0, s, jd, t, theta, L, d);
      else hipLaunchKernelGGL((k_ode_bwd<H, K, M, 1, false, true>), grid, block, 0, s, jobs, t, theta, L, d);
      break;
    default: return XW_E_ARG;
  }
  return xw_launch_status();
}
#endif
template <int H, int K, int M>
int old_launch_fwd(int method, const FwdJobs& jobs, const double* t, const double* theta, int L, int d, hipStream_t s) {
  const dim3 grid(jobs.tile0[jobs.n]), block(64);
  bool act = true;                                     // all jobs or none, all in the same mode (checked by the caller)
  for (int i = 0; i < jobs.n; ++i) act = act && jobs.act[i] != nullptr;
  const int sel = method * 3 + (act ? (jobs.x_only ? 2 : 1) : 0);
  int rc;
  if (old_launch_fwd_narrow<H, K, M>(sel, jobs, t, theta, L, d, grid, s, rc)) return rc;
  switch (sel) {
    case 0: hipLaunchKernelGGL((k_ode_fwd<H, K, M, 0, 0>), grid, block, 0, s, jobs, t, theta, L, d); break;
    case 1: hipLaunchKernelGGL((k_ode_fwd<H, K, M, 0, 1>), grid, block, 0, s, jobs, t, theta, L, d); break;
    case 2: hipLaunchKernelGGL((k_ode_fwd<H, K, M, 0, 2>), grid, block, 0, s, jobs, t, theta, L, d); break;
    case 3: hipLaunchKernelGGL((k_ode_fwd<H, K, M, 1, 0>), grid, block, 0, s, jobs, t, theta, L, d); break;
    case 4: hipLaunchKernelGGL((k_ode_fwd<H, K, M, 1, 1>), grid, block, 0, s, jobs, t, theta, L, d); break;
    case 5: hipLaunchKernelGGL((k_ode_fwd<H, K, M, 1, 2>), grid, block, 0, s, jobs, t, theta, L, d); break;
    case 6: hipLaunchKernelGGL((k_ode_fwd<H, K, M, 2, 0>), grid, block, 0, s, jobs, t, theta, L, d); break;
    default: return XW_E_ARG;
  }
  return xw_launch_status();
}
}  // namespace
#ifndef XW_ODE_PART_RECOMP
static int old_fwd_multi_w(const XwOdeFwdJob* jobs, int njobs, const double* t, const double* theta, int method,
                                             int L, int d, int m, double* zero16, void* stream) {
  if (!jobs || njobs < 1 || njobs > XW_MAXJOBS || !t || !theta || L <= 0 || d <= 0 || m < 1) return XW_E_ARG;
  FwdJobs J;
  J.n = njobs;
  J.zero16 = zero16;
  J.x_only = jobs[0].act_x_only ? 1 : 0;
  J.narrow = jobs[0].narrow ? 1 : 0;
  J.prio = XW_ODE_PRIO - (jobs[0].prio_drop < 0 ? 0 : jobs[0].prio_drop > 3 ? 3 : jobs[0].prio_drop);
  J.tile0[0] = 0;
  for (int i = 0; i < XW_MAXJOBS; ++i) {
    const bool on = i < njobs;
    if (on && (!jobs[i].xT || !jobs[i].start || !jobs[i].u || jobs[i].N <= 0)) return XW_E_ARG;
    if (on && (jobs[i].act_x_only ? 1 : 0) != J.x_only) return XW_E_ARG;         // one store mode per launch
    if (on && (jobs[i].narrow ? 1 : 0) != J.narrow) return XW_E_ARG;              // one layout per launch
    J.xT[i] = on ? jobs[i].xT : nullptr;
    J.start[i] = on ? jobs[i].start : nullptr;
    J.u[i] = on ? jobs[i].u : nullptr;
    J.Y[i] = on ? jobs[i].Y : nullptr;
    J.act[i] = (on && method != 2) ? jobs[i].act : nullptr;     // (rk4 sweeps recompute: nothing to store)
    if (on && (J.act[i] != nullptr) != (J.act[0] != nullptr)) return XW_E_ARG;   // all groups of a launch, or none
    J.N[i] = on ? jobs[i].N : 0;
    J.tile0[i + 1] = J.tile0[i] + (on ? (jobs[i].N + 15) / 16 : 0);
  }
  hipStream_t s = (hipStream_t)stream;
#define CALL(HH, KK, MM) return old_launch_fwd<HH, KK, MM>(method, J, t, theta, L, d, s);
  OLD_ODE_DISPATCH(CALL)
#undef CALL
}

static int old_bwd_multi_w(const XwOdeBwdJob* jobs, int njobs, const double* t, const double* theta, int method,
                                             int L, int d, int m, int mode, void* stream) {
  if (!jobs || njobs < 1 || njobs > XW_MAXJOBS || !t || !theta || L <= 0 || d <= 0 || m < 1 || (mode & 3) == 0 || ((mode & 4) && (mode & 3) != 3) || ((mode & 8) && (mode & 4)) || ((mode & 16) && (mode & 8)) || (mode & ~127)) return XW_E_ARG;
  BwdJobs J;
  J.n = njobs;
  J.x_ones = (mode & 4) ? 1 : 0;
  J.spread = 0;
  J.prio = XW_ODE_PRIO - ((mode >> 5) & 3);
  J.tile0[0] = 0;
  for (int i = 0; i < XW_MAXJOBS; ++i) {
    const bool on = i < njobs;
    if (on && (!jobs[i].Y || !sweep_job_ok(jobs[i], mode))) return XW_E_ARG;      // (xw_generic_cot.h: as every family's entry point)
    if (on && (mode & 1) && (!jobs[i].gx != !jobs[i].gs)) return XW_E_ARG;
    J.xT[i] = on ? jobs[i].xT : nullptr;
    J.start[i] = on ? jobs[i].start : nullptr;
    J.Y[i] = on ? jobs[i].Y : nullptr;
    J.act[i] = (on && method != 2 && !(mode & 8)) ? jobs[i].act : nullptr;   // (rk4 and the continuous adjoint recompute)
    if (on && (J.act[i] != nullptr) != (J.act[0] != nullptr)) return XW_E_ARG;   // all groups of a launch, or none
    J.ubar[i] = on ? jobs[i].ubar : nullptr;
    J.res_u[i] = on ? jobs[i].res_u : nullptr;
    J.res_ref[i] = on ? jobs[i].res_ref : nullptr;
    J.res_coef[i] = on ? jobs[i].res_coef : 0.0;
    J.res_base[i] = on ? jobs[i].res_base : 0.0;
    J.res_first[i] = on ? jobs[i].res_first_only : 0;
    J.res_w[i] = on ? jobs[i].res_w : nullptr;
    J.res_c[i] = on ? jobs[i].res_c : nullptr;
    J.res_cp[i] = on ? jobs[i].res_cp : nullptr;
    J.res_kappa2[i] = on ? jobs[i].res_kappa2 : 0.0;
    J.res_wpp[i] = on ? jobs[i].res_w_per_point : 0;
    J.res_scal[i] = on ? jobs[i].res_scal : nullptr;
    J.res_refA[i] = on ? jobs[i].res_refA : nullptr;
    J.res_coefA[i] = on ? jobs[i].res_coefA : 0.0;
    J.res_baseA[i] = on ? jobs[i].res_baseA : 0.0;
    J.gx[i] = (on && (mode & 1)) ? jobs[i].gx : nullptr;
    J.gs[i] = (on && (mode & 1)) ? jobs[i].gs : nullptr;
    J.gslab[i] = (on && (mode & 2)) ? jobs[i].gslab : nullptr;
    J.N[i] = on ? jobs[i].N : 0;
    J.tile0[i + 1] = J.tile0[i] + (on ? (jobs[i].N + 15) / 16 : 0);
  }
  hipStream_t s = (hipStream_t)stream;
#define CALL(HH, KK, MM)                                                             \
  return (mode & 2) ? old_launch_bwd<HH, KK, MM, true>(method, J, t, theta, L, d, (mode & 8) != 0, (mode & 16) != 0, s)     \
                    : old_launch_bwd<HH, KK, MM, false>(method, J, t, theta, L, d, (mode & 8) != 0, (mode & 16) != 0, s);
  OLD_ODE_DISPATCH(CALL)
#undef CALL
}
#else   // XW_ODE_PART_RECOMP: only the sweeps that re-evaluate the field (no activation store) and the continuous adjoint
static int old_recomp_w(const void* jobs_, const double* t, const double* theta, int method, int L, int d,
                                              int m, int params, int adj, void* stream) {
  const BwdJobs& jobs = *static_cast<const BwdJobs*>(jobs_);
  const dim3 grid(jobs.tile0[jobs.n]), block(64);
  hipStream_t s = (hipStream_t)stream;
#define LAUNCH(HH, KK, MM, PP, AA)                                                                                                 \
  switch (method) {                                                                                                                \
    case 0: hipLaunchKernelGGL((k_ode_bwd<HH, KK, MM, 0, PP, false, AA>), grid, block, 0, s, jobs, t, theta, L, d); break;         \
    case 1: hipLaunchKernelGGL((k_ode_bwd<HH, KK, MM, 1, PP, false, AA>), grid, block, 0, s, jobs, t, theta, L, d); break;         \
    case 2: hipLaunchKernelGGL((k_ode_bwd<HH, KK, MM, 2, PP, false, AA>), grid, block, 0, s, jobs, t, theta, L, d); break;         \
    default: return XW_E_ARG;                                                                                                      \
  }                                                                                                                                \
  return xw_launch_status();
#define CALL(HH, KK, MM)                                                                                                           \
  if (params && adj) { LAUNCH(HH, KK, MM, true, true) }                                                                            \
  else if (params) { LAUNCH(HH, KK, MM, true, false) }                                                                             \
  else if (adj) { LAUNCH(HH, KK, MM, false, true) }                                                                                \
  else { LAUNCH(HH, KK, MM, false, false) }
  OLD_ODE_DISPATCH(CALL)
#undef CALL
#undef LAUNCH
}
#endif
