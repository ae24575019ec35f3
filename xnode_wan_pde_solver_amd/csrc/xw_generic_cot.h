// xw_generic_cot.h -- the cotangent on u of a sweep job (XwOdeBwdJob: stored, all ones or a residual form), per path.
// Library-internal; included INSIDE an anonymous namespace, after xw_generic_field.h.
#pragma once
// cotangent on u at (l, path): stored, all ones, or one of the residual forms of XwOdeBwdJob
__device__ double cot_u(const XwOdeBwdJob& j, int l, int L, int path) {
  const long p = (long)l * j.N + path;
  if (j.res_u == nullptr) return j.ubar ? j.ubar[p] : 1.0;
  if (j.res_first_only == 2) {
    const double u = j.res_u[p], v = j.res_ref[p];
    const double w = j.res_w_per_point ? j.res_w[p] : j.res_w[path];
    const double dcu = j.res_c != nullptr ? j.res_c[p] + u * j.res_cp[p] : j.res_kappa2 * u;
    double g = j.res_coef * dcu * v * w;
    if (l == L - 1) g += j.res_base * v;
    return g;
  }
  if (j.res_first_only == 1) return l == 0 ? j.res_base + j.res_coef * (j.res_u[p] - j.res_ref[path]) : j.res_base;
  return j.res_base + j.res_coef * (j.res_u[p] - j.res_ref[p]);
}
