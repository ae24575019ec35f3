// xw_ode_abi.hip -- public entry points of the stepper (include/xnwan.h): argument checks that do not depend on the
// width, and the choice of the objects compiled for (H, K) (xw_ode_fwd.h, xw_ode.hip; the Makefile has the objects per width).
#include "xw_common.h"
#include "xnwan.h"
#include "xw_generic.h"

/* the containers (keep in step with the Makefile and kernels.ODE_WIDTHS): (20, 10) and (32, 12) on v_mfma_f64_4x4x4 (xw_ode_mfma4.h),
 * the WIDE container (64, 16) on v_mfma_f64_16x16x4 (round 6; -DXW_ODE_WIDE16, xw_ode_mfma16.h: one wave per tile, no
 * narrow tiles); depths 1..10 and the same entry points in all of them */
#define XW_ODE_WIDTHS(X) X(20, 10) X(32, 12) X(64, 16)

#define DECL(H, K)                                                                                                         \
  extern "C" int xw_ode_fwd_multi_w##H##_##K(const XwOdeFwdJob*, int, const double*, const double*, int, int, int, int, double*, void*); \
  extern "C" int xw_ode_bwd_multi_w##H##_##K(const XwOdeBwdJob*, int, const double*, const double*, int, int, int, int, int, void*);
XW_ODE_WIDTHS(DECL)
#undef DECL

extern "C" int xw_ode_bwd_slabs(int N) { return (N + 15) / 16; }

static bool width_compiled(int H, int K) {
#define TEST(HH, KK) if (H == HH && K == KK) return true;
  XW_ODE_WIDTHS(TEST)
#undef TEST
  return false;
}

extern "C" int xw_ode_act_rows(int method, int H, int K, int m) {
  if ((!width_compiled(H, K) || m > XW_ODE_MAX_LAYERS) && xwg_ode_ok(1, H, K, m)) return 0;   // generic widths / depths (xw_generic.hip): the sweeps recompute
  if (!width_compiled(H, K) || m < 1 || m > XW_ODE_MAX_LAYERS) return XW_E_DIMS;
  const int S = method == 0 ? 1 : method == 1 ? 2 : 0;           // rk4: the sweeps recompute
  // layer inputs + the stage inputs + the ReLU-mask words of every stage: (K + 3) / 4 bits per layer and lane, two rows per 32-bit
  // word (XW_MASK_WORDS of xw_ode_core.h: a second word only in the wide container at depth 10)
  const int w = ((K + 3) / 4) * (m - 1) > 32 ? 4 : 2;
  return S == 0 ? 0 : S * m * K + (S - 1) * H + w * S;
}

extern "C" int xw_ode_fwd_multi(const XwOdeFwdJob* jobs, int njobs, const double* t, const double* theta, int method, int L,
                                int d, int H, int K, int m, double* zero16, void* stream) {
  if (method < 0 || method > 2) return XW_E_ARG;    // fixed-grid ids 0..2 only (dopri5, explicit_adams: entry points of their own)
#define CALL(HH, KK) if (H == HH && K == KK && m <= XW_ODE_MAX_LAYERS) return xw_ode_fwd_multi_w##HH##_##KK(jobs, njobs, t, theta, method, L, d, m, zero16, stream);
  XW_ODE_WIDTHS(CALL)
#undef CALL
  return xwg_ode_fwd_multi(jobs, njobs, t, theta, method, L, d, H, K, m, zero16, stream);    // any other width: the generic path
}

extern "C" int xw_ode_fwd(const double* xT, const double* t, const double* start, const double* theta, int method, int N,
                          int L, int d, int H, int K, int m, double* u, double* Y, void* stream) {
  XwOdeFwdJob j = {xT, start, u, Y, nullptr, N, 0, 0, 0};
  return xw_ode_fwd_multi(&j, 1, t, theta, method, L, d, H, K, m, nullptr, stream);
}

extern "C" int xw_ode_bwd_multi(const XwOdeBwdJob* jobs, int njobs, const double* t, const double* theta, int method, int L,
                                int d, int H, int K, int m, int mode, void* stream) {
  if (method < 0 || method > 2) return XW_E_ARG;
#define CALL(HH, KK) if (H == HH && K == KK && m <= XW_ODE_MAX_LAYERS) return xw_ode_bwd_multi_w##HH##_##KK(jobs, njobs, t, theta, method, L, d, m, mode, stream);
  XW_ODE_WIDTHS(CALL)
#undef CALL
  return xwg_ode_bwd_multi(jobs, njobs, t, theta, method, L, d, H, K, m, mode, stream);
}

extern "C" int xw_ode_bwd(const double* xT, const double* t, const double* start, const double* theta, const double* Y,
                          const double* ubar, int method, int N, int L, int d, int H, int K, int m, int mode, double* gx,
                          double* gs, double* gslab, void* stream) {
  XwOdeBwdJob j = {xT, start, Y, nullptr, ubar, gx, gs, gslab, N, 0, nullptr, nullptr, 0.0, 0.0, 0, nullptr, nullptr, nullptr, 0.0};
  return xw_ode_bwd_multi(&j, 1, t, theta, method, L, d, H, K, m, mode, stream);
}
