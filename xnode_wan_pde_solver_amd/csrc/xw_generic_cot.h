// xw_generic_cot.h -- the cotangent on u of a sweep job (XwOdeBwdJob: stored, all ones or a residual form), per path, and the
// host side's check of such a job.  Library-internal; included INSIDE an anonymous namespace, after xw_common.h and xnwan.h.
#pragma once
// the weak form's dI/du at (l, path) -- kind 2, and the B part of kind 3
__device__ __forceinline__ double cot_weak(const XwOdeBwdJob& j, int l, int L, int path, long p) {
  const double u = j.res_u[p], v = j.res_ref[p];
  const double w = j.res_w_per_point ? j.res_w[p] : j.res_w[path];
  const double dcu = j.res_c != nullptr ? j.res_c[p] + u * j.res_cp[p] : j.res_kappa2 * u;
  return xw_cot_weak(j.res_coef, j.res_base, dcu, v, w, l == L - 1);
}
// cotangent on u at (l, path): stored, all ones, or one of the residual forms of XwOdeBwdJob
__device__ double cot_u(const XwOdeBwdJob& j, int l, int L, int path) {
  const long p = (long)l * j.N + path;
  if (j.res_u == nullptr) return j.ubar ? j.ubar[p] : 1.0;
  // merged: kind 1 with the A fields + (2 / I) kind 2.  Accepted here: res_scal[0] is loaded and 2 / I divided at EVERY
  // (l, path) call, not once per wave in front of the time loop as the fused containers do (xw_ode_core.h, make_cot) -- the
  // families behind this header (generic, tiled, both dopri5 steppers) call cot_u from thirteen places in five kernels, none of
  // them on the headline path, and the same quotient of the same two doubles gives the same bits wherever it is formed.
  if (j.res_first_only == 3)
    return xw_cot_merged(xw_cot_init(j.res_baseA, j.res_coefA, j.res_u[p], j.res_refA[path], l == 0), 2.0 / j.res_scal[0],
                         cot_weak(j, l, L, path, p));
  if (j.res_first_only == 2) return cot_weak(j, l, L, path, p);
  if (j.res_first_only == 1) return xw_cot_init(j.res_base, j.res_coef, j.res_u[p], j.res_ref[path], l == 0);
  return j.res_base + j.res_coef * (j.res_u[p] - j.res_ref[p]);
}
// host side: the residual fields of a job are a form the sweeps know (every family's entry point asks)
inline bool cot_job_ok(const XwOdeBwdJob& j) {
  if (j.res_first_only < 0 || j.res_first_only > 3) return false;
  if (j.res_u == nullptr) return j.res_first_only != 3;
  if (j.ubar != nullptr || j.res_ref == nullptr) return false;
  if (j.res_first_only >= 2 && (j.res_w == nullptr || (!j.res_c != !j.res_cp))) return false;
  if (j.res_first_only == 3 && (j.res_scal == nullptr || j.res_refA == nullptr)) return false;
  return true;
}
// host side: is this sweep job well-formed for `mode` (bit 0: x-side outputs, bit 1: parameter gradients, bit 2: all-ones x cotangent)?
// (the state the sweep reverses -- Y, or the dopri5 record -- is the caller's to check)
inline bool sweep_job_ok(const XwOdeBwdJob& j, int mode) {
  if (!j.xT || !j.start || j.N < 1 || !cot_job_ok(j)) return false;
  if ((mode & 2) && !j.gslab) return false;
  return !((mode & 1) && !(mode & 4) && (!j.gx || !j.gs));
}
