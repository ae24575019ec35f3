/* xnwan_grad.h -- extension of the C ABI of libxnwan.so (include/xnwan.h, which stays as it is): the gradient and the time
 * derivative of u at scattered space-time points, a reverse sweep over a RAGGED group with a time grid per path
 * (csrc/xw_tiled_paths_grad.hip).  Conventions as in xnwan.h: device pointers owned by the caller, `stream` a hipStream_t,
 * 0 = ok / negative XW_E_* / positive hipError_t.
 *
 * A job is a job of xw_paths_tiled_fwd (xnwan.h) after that forward pass: path p has the spatial point xT[.][p] ([d][N]), the start
 * value start[p], its own non-decreasing times tT[l][p], l < L ([L][N]; a shorter path repeats its last time) and the checkpoints
 * Y[L][H][N] the forward pass wrote (NOT last_only); nstep[N] (may be NULL) is the forward's hint, the index of each path's last
 * distinct time.  The forward is never recomputed.  With u_p = FL(y_{n_p}), the forward's final value of path p:
 *   gx[d][N] : du_p/dx_p with the start value and the path's grid held fixed
 *   gs[N]    : du_p/dstart_p
 *              -- both the DISCRETE adjoint: the exact reverse of the steps taken (method 0 euler, 1 midpoint, 2 rk4 by the 3/8
 *              rule), step sizes as constants; what autograd through the reference's fixed-grid odeint gives for the one-path job
 *   ut[N]    : FL_w . F(t_p, x_p, y(t_p)) at the path's last time and final state -- the time derivative of the CONTINUOUS model
 *              y' = F, u = FL y at fixed x.  It is NOT the derivative of the discrete u with respect to the end time of its grid:
 *              that would need d(step)/d(dt), which nothing here builds.
 * gx, gs and ut may each be NULL, not all three.  One wave per 16-path tile walks min(L - 1, max nstep over the tile) steps back from
 * a cotangent 1 on every path's final value; a zero-length step is the exact identity of the reverse, so a path's bits do not
 * depend on the paths beside it.  No float atomics, no waits between tiles, no host read-back: the launch can be captured.
 * work: xw_paths_tiled_grad_work(d, H, K, m) doubles per 16-path tile -- the tiled sweep's, xw_tiled_ode_work(1, ...) -- times the
 * launch's tiles, the sum over the jobs of (N + 15) / 16, in job order.
 * Refused on the host before any launch: XW_E_ARG for null pointers (jobs, theta, work, a job's xT, start, tT, Y; gx, gs and ut all
 * null), njobs < 1, N < 1, L < 1, a method outside 0..2; XW_E_DIMS where xw_tiled_ode_ok(d, H, K, m) is 0. */
#ifndef XNWAN_GRAD_H
#define XNWAN_GRAD_H
#include "xnwan.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct { const double* xT; const double* start; const double* tT; const int* nstep;
                 const double* Y; double* gx; double* gs; double* ut; int N; } XwPathsGradJob;
int xw_paths_tiled_grad_work(int d, int H, int K, int m);   /* doubles per 16-path tile == xw_tiled_ode_work(1, ...) */
int xw_paths_tiled_grad(const XwPathsGradJob* jobs, int njobs, const double* theta, int method, int L,
                        int d, int H, int K, int m, double* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif
